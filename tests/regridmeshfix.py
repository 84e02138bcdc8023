"""TEST INFRASTRUCTURE for the tests of resuming a refined run on other cuts (test_regrid_mesh.py, test_gpu_regrid_mesh.py):
reads tests/golden/regridmesh_*.npz (written by tests/golden/make_golden_regrid_mesh.py from runs of the reference built with MPI
and static mesh refinement, every <domainN> cut differently) and joins the seed files in plain numpy by the reference's rules,
written out here independently of restart.mesh_grid_boxes / box_pieces:
  A  every Domain, level by level, is cut by its own NGrid_x* into Grids of Nx / NGrid zones, the remainder on the first Grid;
  B  the Grids take consecutive ranks, x1 fastest, the count running on from Domain to Domain and wrapping at the rank count;
  C  rank r's file holds the sections of its Grids in that order.
EdgeFlux: a face two Grids share is the upper Grid's, the last face of a direction the last Grid's."""
import json
import os
import struct

import numpy as np

from dumpfix import GOLDEN, pkg

LABELS = ("DENSITY", "1-MOMENTUM", "2-MOMENTUM", "3-MOMENTUM", "ENERGY")
CASES = ["blast2_x1x3", "blast2_noroot", "blast3_uneven", "sphere2_x2x3", "sphere2_x1", "blast2dom"]
CONTINUED_BLAST = ["blast2_x1x3", "blast2_noroot", "blast3_uneven"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def split_payload(b):
    """(parameter dump as text, everything behind the line of <par_end>) of a restart file's bytes"""
    end = b.index(b"\n", b.index(b"<par_end>")) + 1
    return b[:end].decode(errors="replace"), b[end:]


class RMFixture:
    def __init__(self, name):
        self.name = name
        self.z = z = np.load(os.path.join(GOLDEN, "regridmesh_" + name + ".npz"))
        self.problem = str(z["problem"])
        self.nranks = int(z["nranks"])
        self.blocks = json.loads(str(z["blocks"]))
        self.domains = [(int(d[0]), tuple(int(v) for v in d[1:4]), tuple(int(v) for v in d[4:7])) for d in z["domains"]]
        self.Nxs = [d[1] for d in self.domains]
        self.ngrid = [tuple(int(v) for v in g) for g in z["ngrid"]]
        self.seed_names = [str(p) for p in z["seed_names"]]
        self.seed_nstep, self.seed_time, self.seed_dt = int(z["seed_nstep"]), float(z["seed_time"]), float(z["seed_dt"])
        self.nscal = 1 if self.problem == "ioniz_sphere" else 0
        self.ion = self.problem != "blast"
        self.continued = "final_nstep" in z.files
        if self.continued:
            self.nlim = int(z["nlim"])
            self.resume_overrides = ["time/nlim=%d" % self.nlim]      # (the seeds' table carries the nlim their run stopped at)
            self.final_time, self.final_dt, self.final_nstep = float(z["final_time"]), float(z["final_dt"]), int(z["final_nstep"])
            self.niter = [[int(v) for v in row] for row in z["niter"]]

    def seed_bytes(self, i):
        return self.z[f"seed_{i}"].tobytes()

    def write_seeds(self, d, by_rank=True, skip=()):
        """the seed files under `d` (by_rank: id<r>/ as the ranks left them, else side by side) -> rank 0's path"""
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

    # ---- the rules, once more ----
    def dealt(self):
        """per Domain [(rank, lo, nx)], lo relative to the Domain"""
        out, nxt = [], 0
        for (_lev, Nx, _disp), ng in zip(self.domains, self.ngrid):
            sz, dp = [], []
            for d in range(3):
                q, r = divmod(Nx[d], ng[d])
                s = [q + r] + [q] * (ng[d] - 1)
                sz.append(s); dp.append([sum(s[:i]) for i in range(ng[d])])
            row = []
            for n in range(ng[2]):
                for m in range(ng[1]):
                    for l in range(ng[0]):
                        row.append((nxt, (dp[0][l], dp[1][m], dp[2][n]), (sz[0][l], sz[1][m], sz[2][n])))
                        nxt = (nxt + 1) % self.nranks
            out.append(row)
        assert nxt == 0
        return out

    def parse(self, b, nxs):
        """[(U, ef)] of the Grids of `nxs` zones in a restart file's bytes, which must hold exactly those"""
        pos = b.index(b"\nTIME_STEP\n") + 11 + 8
        out = []
        for nx in nxs:
            n = nx[0] * nx[1] * nx[2]
            U = np.zeros((nx[2], nx[1], nx[0], 5 + self.nscal)); ef = None
            labels = list(LABELS) + (["EDGEFLUX"] if self.ion else []) + [f"SCALAR {s}" for s in range(self.nscal)]
            for lab in labels:
                tag = b"\n" + lab.encode() + b"\n"
                assert b[pos:pos + len(tag)] == tag, (lab, b[pos:pos + 16])
                pos += len(tag)
                if lab == "EDGEFLUX":
                    ne = (nx[0] + 1) * (nx[1] + 1) * (nx[2] + 1)
                    ef = np.frombuffer(b, "<f8", ne, pos).reshape(nx[2] + 1, nx[1] + 1, nx[0] + 1).copy(); pos += 8 * ne
                else:
                    c = LABELS.index(lab) if lab in LABELS else 5 + int(lab.split()[1])
                    U[..., c] = np.frombuffer(b, "<f8", n, pos).reshape(nx[2], nx[1], nx[0]); pos += 8 * n
            out.append((U, ef))
        assert b[pos:] == b"\nUSER_DATA\n"
        return out

    def head(self, b):
        pos = b.index(b"N_STEP\n", b.index(b"<par_end>")) + 7
        nstep = struct.unpack_from("<i", b, pos)[0]
        time = struct.unpack_from("<d", b, pos + 4 + 6)[0]
        dt = struct.unpack_from("<d", b, pos + 4 + 6 + 8 + 11)[0]
        return nstep, time, dt

    def join_files(self, file_bytes):
        """[(U, ef)] per Domain from the bytes of the files of all ranks (rank order)"""
        table = self.dealt()
        grids = {}
        for r, b in enumerate(file_bytes):
            mine = [(n, box) for n, row in enumerate(table) for box in row if box[0] == r]
            for (n, _box), st in zip(mine, self.parse(b, [box[2] for _n, box in mine])):
                grids[(n, r)] = st
        out = []
        for n, ((_lev, Nx, _disp), row) in enumerate(zip(self.domains, table)):
            U = np.zeros((Nx[2], Nx[1], Nx[0], 5 + self.nscal)); cover = np.zeros((Nx[2], Nx[1], Nx[0]), dtype=int)
            ef = np.zeros((Nx[2] + 1, Nx[1] + 1, Nx[0] + 1)) if self.ion else None
            for rank, lo, nx in sorted(row, key=lambda t: (t[1][2], t[1][1], t[1][0])):       # lower Grids first
                Ug, eg = grids[(n, rank)]
                U[lo[2]:lo[2] + nx[2], lo[1]:lo[1] + nx[1], lo[0]:lo[0] + nx[0]] = Ug
                cover[lo[2]:lo[2] + nx[2], lo[1]:lo[1] + nx[1], lo[0]:lo[0] + nx[0]] += 1
                if self.ion:
                    ef[lo[2]:lo[2] + nx[2] + 1, lo[1]:lo[1] + nx[1] + 1, lo[0]:lo[0] + nx[0] + 1] = eg
            assert np.all(cover == 1)
            out.append((U, ef))
        return out

    def joined_seeds(self):
        return self.join_files([self.seed_bytes(i) for i in range(self.nranks)])

    def final(self):
        return [(self.z[f"final_U{n}"], self.z[f"final_EF{n}"] if self.ion else None) for n in range(len(self.domains))]


def check_split_files(fx, rundir, written):
    """the files a run wrote with rst_mesh_ngrid = fx's cuts: the bytes behind <par_end> are the seed files'; the tables agree as
    parsed in NGrid_x* of every Domain, problem_id, every block's num / time and <time> time"""
    A = pkg("athinput")
    assert sorted(written) == sorted(fx.seed_names), (written, fx.seed_names)
    base = None
    for i, rel in enumerate(fx.seed_names):
        head, payload = split_payload(open(os.path.join(rundir, rel), "rb").read())
        rhead, rpayload = split_payload(fx.seed_bytes(i))
        assert payload == rpayload, rel
        a, b = A.ParTable.from_text(head), A.ParTable.from_text(rhead)
        for n, ng in enumerate(fx.ngrid, 1):
            for k in (1, 2, 3):
                assert a.geti(f"domain{n}", f"NGrid_x{k}") == b.geti(f"domain{n}", f"NGrid_x{k}") == ng[k - 1], (rel, n, k)
            assert not a.exist(f"domain{n}", "AutoWithNProc")
        for k in fx.blocks:
            assert a.geti(f"output{k}", "num") == b.geti(f"output{k}", "num") and a.getd(f"output{k}", "time") == b.getd(f"output{k}", "time")
        base = base or b.gets("job", "problem_id")
        assert a.gets("job", "problem_id") == b.gets("job", "problem_id") == base + ("-id%d" % i if i else "")
        assert a.getd("time", "time") == b.getd("time", "time")


# ---- the reference continues from files this package wrote ------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from refmpi import MPIEXEC      # noqa: E402  (where the tests that run the reference's MPI builds find mpiexec)
REF_EXE = os.path.join(ROOT, "oracle", "_ref", "athena_blast_smr_mpi")


def reference_available():
    return os.path.exists(REF_EXE) and os.path.exists(MPIEXEC)


def reference_continues(files, nlim, rundir):
    """``mpiexec -n N athena_blast_smr_mpi -r <rank 0's file> time/nlim=nlim`` (the reference's MPI + SMR build under oracle/_ref,
    one CPU-only child) from `files`, the restart dumps of the N ranks in rank order -- put side by side first: the reference's
    ranks look for their files next to rank 0's (main.c:265-288).  -> the bytes of the last restart dump of every rank, in rank
    order"""
    import shutil
    import subprocess
    nranks = len(files)
    flat = rundir + "_seeds"
    os.makedirs(flat)
    for f in files:
        shutil.copy(f, flat)
    path0 = os.path.join(flat, os.path.basename(files[0]))
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/conda/lib:" + env.get("LD_LIBRARY_PATH", "")
    pr = subprocess.run([MPIEXEC, "-n", str(nranks), REF_EXE, "-r", path0, "-d", rundir, "time/nlim=%d" % nlim],
                        stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=os.path.dirname(rundir), env=env, timeout=120)
    assert pr.returncode == 0, pr.stdout[-1500:] + pr.stderr[-1500:]
    out = []
    for r in range(nranks):
        d = os.path.join(rundir, "id%d" % r)
        out.append(open(os.path.join(d, sorted(f for f in os.listdir(d) if f.endswith(".rst"))[-1]), "rb").read())
    return out
