"""TEST INFRASTRUCTURE for the tests of resuming on another decomposition (test_regrid.py, test_gpu_regrid.py): reads
tests/golden/regrid_*.npz (written by tests/golden/make_golden_regrid.py from runs of the reference's MPI executables on cuts this
package never runs on) and joins per-Grid arrays in plain numpy, independently of restart.box_pieces."""
import os
import re

import numpy as np

import dumpfix
from dumpfix import pkg

FIXTURES = ["regrid_blast_x1x3_16x12x8_s3_s8", "regrid_blast_uneven_22x12x9_s3_s6", "regrid_ioniz_sphere_x1x2_24x20x16_s6_s10"]


class GFixture(dumpfix.Fixture):
    def __init__(self, name):
        super().__init__(name)
        z = self.z
        self.ngrid = tuple(int(v) for v in z["ngrid"])
        self.seed_names = [str(p) for p in z["seed_names"]]
        self.niter = [int(v) for v in z["niter"]]
        self.seed_nstep, self.seed_time, self.seed_dt = int(z["seed_nstep"]), float(z["seed_time"]), float(z["seed_dt"])
        self.ion = self.problem != "blast"
        self.seed_join_equal = bool(z["seed_join_equal"])
        self.ef_shared_equal = bool(z["ef_shared_equal"])

    def par(self):
        """our deck with the run's blocks, and the reference run's box (the sphere's fixtures zoom in)"""
        return super().par().cmdline([str(o) for o in self.z["overrides"] if str(o).startswith("domain1/x")])

    def seed_bytes(self, i):
        return self.z[f"seed_{i}"].tobytes()

    def write_seeds(self, d, by_rank=False, skip=()):
        """as restartfix.RFixture.write_seeds; -> rank 0's path"""
        first = None
        for i, rel in enumerate(self.seed_names):
            if i in skip:
                continue
            p = os.path.join(d, rel if by_rank else os.path.basename(rel))
            os.makedirs(os.path.dirname(p), exist_ok=True)
            with open(p, "wb") as f:
                f.write(self.seed_bytes(i))
            if i == 0:
                first = p
        return first

    def vtk_grid(self, r):
        """(nx, origin) of rank r's Grid as its vtk header states them (DIMENSIONS counts the faces)"""
        h = str(self.z[f"vtkhead_{r}"])
        dims = [int(v) - 1 for v in re.search(r"DIMENSIONS (\d+) (\d+) (\d+)", h).groups()]
        org = [float(v) for v in re.search(r"ORIGIN (\S+) (\S+) (\S+)", h).groups()]
        return tuple(dims), tuple(org)

    def vtk_boxes(self):
        """[(disp, nx)] per rank from the vtk headers alone: the origin in zones of the root Domain"""
        run = self.run_config()
        out = []
        for r in range(self.nranks):
            nx, org = self.vtk_grid(r)
            disp = tuple(int(round((org[d] - run.xmin[d]) / run.dx[d])) for d in range(3))
            for d in range(3):                   # (%e prints seven digits)
                assert abs(run.xmin[d] + disp[d] * run.dx[d] - org[d]) <= 1e-6 * max(abs(run.xmax[d]), abs(run.xmin[d])), (r, d, org)
            out.append((disp, nx))
        return out

    def seed_states(self, tmpdir):
        """[(U, edgeflux)] of every rank's seed, read with the whole-file reader restart.read_rst on the vtk headers' sizes"""
        R = pkg("restart")
        out = []
        for i, (_disp, nx) in enumerate(self.vtk_boxes()):
            p = os.path.join(tmpdir, f"seed_state_{i}.rst")
            with open(p, "wb") as f:
                f.write(self.seed_bytes(i))
            r = R.read_rst(p, nx, self.nscal, self.ion)
            out.append((r["U"][..., :5 + self.nscal], r["edgeflux"]))
        return out

    def final_states(self):
        return [(self.z[f"final_{r}_U"][..., :5 + self.nscal], self.z[f"final_{r}_EF"] if self.ion else None) for r in range(self.nranks)]


def join(states, boxes, nx, lo=(0, 0, 0), n=None):
    """The part [lo, lo + n) of the root Domain from per-Grid (U, edgeflux) and their (disp, nx): every Grid pasted into the whole
    Domain, lower Grids first -- so that a face two Grids share holds the UPPER Grid's entry and the last face of a direction the
    last Grid's -- and the part cut out."""
    n = n or nx
    nv = states[0][0].shape[-1]
    U = np.zeros((nx[2], nx[1], nx[0], nv)); ef = None
    if states[0][1] is not None:
        ef = np.zeros((nx[2] + 1, nx[1] + 1, nx[0] + 1))
    order = sorted(range(len(boxes)), key=lambda r: (boxes[r][0][2], boxes[r][0][1], boxes[r][0][0]))
    for r in order:
        (d, m), (Ur, er) = boxes[r], states[r]
        U[d[2]:d[2] + m[2], d[1]:d[1] + m[1], d[0]:d[0] + m[0]] = Ur
        if ef is not None:
            ef[d[2]:d[2] + m[2] + 1, d[1]:d[1] + m[1] + 1, d[0]:d[0] + m[0] + 1] = er
    U = U[lo[2]:lo[2] + n[2], lo[1]:lo[1] + n[1], lo[0]:lo[0] + n[0]]
    if ef is not None:
        ef = ef[lo[2]:lo[2] + n[2] + 1, lo[1]:lo[1] + n[1] + 1, lo[0]:lo[0] + n[0] + 1]
    return U, ef


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def split_payload(b):
    """(parameter dump as text, everything behind the line of <par_end>) of a restart file's bytes"""
    end = b.index(b"\n", b.index(b"<par_end>")) + 1
    return b[:end].decode(errors="replace"), b[end:]
