"""TEST INFRASTRUCTURE for the restart tests (test_restart_resume.py, test_gpu_restart.py): reads tests/golden/restart_*.npz (written
by tests/golden/make_golden_restart.py from runs of the reference's own executables that were continued with ``athena -r``) and
compares the tree a resumed run of this package left with the tree the reference's resumed run left."""
import os

import numpy as np

import dumpfix
from dumpfix import pkg

FIXTURES = ["restart_blast_16x12x8_s3_s8", "restart_blast_16x12x8_s3_s11", "restart_blast_mpi2_16x12x8_s3_s8",
            "restart_blast_smr_16x12x8_s2_s5", "restart_ioniz_sphere_24x20x16_s6_s10"]


class RFixture(dumpfix.Fixture):
    def __init__(self, name):
        super().__init__(name)
        z = self.z
        self.seed_names = [str(p) for p in z["seed_names"]]
        self.resume_overrides = [str(a) for a in z["resume_overrides"]]
        self.niter = [int(v) for v in z["niter"]]
        self.seed_nstep, self.seed_time, self.seed_dt = int(z["seed_nstep"]), float(z["seed_time"]), float(z["seed_dt"])
        self.ion = self.problem != "blast"

    def seed_bytes(self, i):
        return self.z[f"seed_{i}"].tobytes()

    def write_seeds(self, d, by_rank=False):
        """the seed file(s) under `d`: all in one directory (where the reference looks), or as the ranks wrote them (id<r>/);
        -> rank 0's path"""
        first = None
        for i, rel in enumerate(self.seed_names):
            p = os.path.join(d, rel if by_rank else os.path.basename(rel))
            os.makedirs(os.path.dirname(p), exist_ok=True)
            with open(p, "wb") as f:
                f.write(self.seed_bytes(i))
            if "-id" not in os.path.basename(rel):
                first = p
        return first

    def level_nx(self, rank=0):
        """active zones of every level a restart dump of `rank` holds, root first"""
        g = self.grids()
        return [g[(rank, l)].Nx for l in range(1 + len(self.levels))]

    def hst(self, rel):
        return str(self.z["hst_%d" % self.paths.index(rel)])


def tree(rundir):
    return sorted(os.path.relpath(os.path.join(dp, f), rundir) for dp, _, fs in os.walk(rundir) for f in fs)


def parse_hst(text):
    lines = text.splitlines()
    return [l for l in lines if l.startswith("#")], np.array([[float(x) for x in l.split()] for l in lines if not l.startswith("#")])


def compare_resumed_tree(fx, rundir, ranks=None, tol=0.0, hst_rows=None):
    """The tree of the reference's resumed run: the same relative paths (so: no file of the forced first output, continued
    numbers); dumps byte for byte (dumpfix.compare_dump); restart dumps equal as parsed -- U and EdgeFlux of every level, time, dt,
    nstep, every block's num / time; .hst files equal as text, without a header.
    tol > 0 (radiation on a GPU): fields within tol of each field's maximum, time and dt to 1e-12, dumps by size only; hst_rows:
    the comparison of the parsed rows where the text may differ in the last printed digit."""
    R = pkg("restart")
    want = [p for p in fx.paths if ranks is None or _rank_of(p) in ranks]
    got = tree(rundir)
    assert got == want, (got, want)
    grids = fx.grids()
    maxout = max(int(k) for k in fx.blocks)
    for i, rel in enumerate(fx.paths):
        if rel not in want:
            continue
        p = os.path.join(rundir, rel)
        if rel.endswith(".hst"):
            text = open(p).read()
            head, rows = parse_hst(text)
            assert head == [], f"{rel}: a resumed run writes no header"
            if hst_rows is None:
                assert text == fx.hst(rel), rel
            else:
                hst_rows(rows, parse_hst(fx.hst(rel))[1])
        elif rel.endswith(".rst"):
            rank = _rank_of(rel)
            nxs = fx.level_nx(rank)
            r = R.scan_rst(p, nxs, fx.nscal, fx.ion)
            assert r["nstep"] == int(fx.z[f"rst_{i}_nstep"]), rel
            t_ref, dt_ref = float(fx.z[f"rst_{i}_time"]), float(fx.z[f"rst_{i}_dt"])
            if tol == 0.0:
                assert r["time"] == t_ref and r["dt"] == dt_ref, (rel, r["time"], t_ref, r["dt"], dt_ref)
            else:
                assert abs(r["time"] / t_ref - 1) < 1e-12 and abs(r["dt"] / dt_ref - 1) < 1e-12, (rel, r["time"], t_ref, r["dt"], dt_ref)
            for l, nx in enumerate(nxs):
                U, ef = R.read_state(r, l, nx, fx.nscal)
                refs = [(U, fx.z[f"rst_{i}_U{l}"][..., :5 + fx.nscal])]
                if fx.ion:
                    refs.append((ef[..., None], fx.z[f"rst_{i}_EF{l}"][..., None]))
                for a, b in refs:
                    if tol == 0.0:
                        assert np.array_equal(a, b), (rel, l)
                    else:
                        scale = np.abs(b).max(axis=(0, 1, 2))
                        assert np.all(a[..., scale == 0] == 0), (rel, l)
                        err = (np.abs(a - b)[..., scale > 0] / scale[scale > 0]).max(axis=(0, 1, 2))
                        print(f"{fx.name}:{rel} level {l}: max error / field maximum {err}")
                        assert err.max() < tol, (rel, l, err)
            nums, nexts = dumpfix.rst_par_values(p, maxout)
            assert nums == [int(v) for v in fx.z[f"rst_{i}_num"]], (rel, nums, fx.z[f"rst_{i}_num"])
            assert nexts == [float(v) for v in fx.z[f"rst_{i}_next"]], (rel, nexts, fx.z[f"rst_{i}_next"])
        else:
            rank, level, _ = fx.where(rel)
            ext = rel.rsplit(".", 1)[1]
            if tol == 0.0:
                dumpfix.compare_dump(open(p, "rb").read(), fx.file(rel), grids[(rank, level)].Nx, fx.nscal, ext, fx.prim_of(ext), f"{fx.name}:{rel}")
            else:
                assert os.path.getsize(p) == len(fx.file(rel)), rel


def _rank_of(rel):
    return int(rel.split("/")[0][2:]) if rel.startswith("id") and "/" in rel else 0
