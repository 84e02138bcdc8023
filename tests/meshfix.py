"""TEST INFRASTRUCTURE for the MeshDriver output tests (test_mesh_driver_outputs.py, test_gpu_mesh_driver_outputs.py): reads
tests/golden/meshdrv_*.npz (written by tests/golden/make_golden_meshdriver.py from two-rank runs of the reference built with
MPI and static mesh refinement), resolves (rank, level) -> GridConfig through config.mesh_slabs, starts the ranks over gloo and
compares the tree a run of this package left with the reference's."""
import os
import socket
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import dumpfix                                         # noqa: E402
from dumpfix import pkg                                # noqa: E402
from restartfix import _rank_of, parse_hst, tree       # noqa: E402
from test_history import check_rows                    # noqa: E402


class MFixture(dumpfix.Fixture):
    """dumpfix.Fixture with ranks AND levels; the seed members of restartfix.RFixture where the fixture holds seeds"""

    def __init__(self, name):
        super().__init__(name)
        z = self.z
        self.ion = self.problem != "blast"
        self.resumed = "seed_names" in z.files
        self.niter = [[int(v) for v in row] for row in z["niter"]] if "niter" in z.files else []
        if self.resumed:
            self.seed_names = [str(p) for p in z["seed_names"]]
            self.resume_overrides = [str(a) for a in z["resume_overrides"]]
            self.seed_nstep, self.seed_time, self.seed_dt = int(z["seed_nstep"]), float(z["seed_time"]), float(z["seed_dt"])
        self._grids = None

    def grids(self):
        """{(rank, level): GridConfig} of the slabs config.mesh_slabs deals (a rank without zones of a level has no entry)"""
        if self._grids is None:
            cfg = pkg("config")
            par = self.par(); run = self.run_config(par)
            self._grids = {(r, g.level): g for r in range(self.nranks) for g in cfg.mesh_slabs(par, run, r, self.nranks).levels}
        return self._grids

    def level_nx(self, rank=0):
        g = self.grids()
        return [g[(rank, l)].Nx for l in range(1 + len(self.levels)) if (rank, l) in g]

    def par(self):
        if self.resumed:                  # the table of the run is the one its seed carries
            import tempfile
            with tempfile.TemporaryDirectory() as d:
                return pkg("restart").read_head(self.write_seeds(d))["par"]
        return super().par()

    def seed_bytes(self, i):
        return self.z[f"seed_{i}"].tobytes()

    def write_seeds(self, d, by_rank=False):
        """as restartfix.RFixture.write_seeds -> rank 0's path"""
        first = None
        for i, rel in enumerate(self.seed_names):
            p = os.path.join(d, rel if by_rank else os.path.basename(rel))
            os.makedirs(os.path.dirname(p), exist_ok=True)
            with open(p, "wb") as f:
                f.write(self.seed_bytes(i))
            if "-id" not in os.path.basename(rel):
                first = p
        return first

    def hst(self, rel):
        return str(self.z["hst_%d" % self.paths.index(rel)])

    def size(self, rel):
        i = self.paths.index(rel)
        return int(self.z[f"size_{i}"]) if f"size_{i}" in self.z.files else len(self.file(rel))


def compare_hst(text, ref_text, mom_rtol=2e-6, what=""):
    """headers character for character (none at all in a resumed run's file), rows by test_history.check_rows"""
    head, rows = parse_hst(text)
    head_ref, rows_ref = parse_hst(ref_text)
    assert head == head_ref, (what, head, head_ref)
    check_rows(rows, rows_ref, mom_rtol=mom_rtol)


def compare_tree(fx, rundir, tol=0.0, mom_rtol=2e-6):
    """The reference's tree: the same relative paths; dumps under dumpfix.compare_dump (byte for byte); restart dumps equal as
    parsed -- U (and EdgeFlux) of every level the rank holds, time, dt, nstep, every block's num / time; .hst by compare_hst.
    tol > 0 (radiation): fields within tol of each field's maximum, time and dt to 1e-12, dumps by size."""
    R = pkg("restart")
    got = tree(rundir)
    assert got == fx.paths, (got, fx.paths)
    grids = fx.grids()
    maxout = max(int(k) for k in fx.blocks)
    for i, rel in enumerate(fx.paths):
        p = os.path.join(rundir, rel)
        if rel.endswith(".hst"):
            compare_hst(open(p).read(), fx.hst(rel), mom_rtol, rel)
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
                if f"rst_{i}_U{l}" not in fx.z.files:
                    continue
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
                assert os.path.getsize(p) == fx.size(rel), rel


# ---- two ranks over gloo ---------------------------------------------------------------------------------------------------
def free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    return port


def _rank_entry(rank, world, port, fn, args, q):
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        q.put((rank, fn(rank, world, *args)))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def run_ranks(fn, args=(), world=2, timeout=300):
    """fn(rank, world, *args) in `world` spawned processes with a gloo group; -> its results in rank order.  `fn` must be a
    module-level function (spawn pickles it by name)."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue(); port = free_port()
    ps = [ctx.Process(target=_rank_entry, args=(r, world, port, fn, args, q)) for r in range(world)]
    for p in ps:
        p.start()
    import queue
    import time
    res, t0 = [], time.monotonic()
    try:
        while len(res) < world:
            try:
                res.append(q.get(timeout=0.5))
            except queue.Empty:             # a rank that died leaves its peer waiting in a collective: do not wait with it
                assert not any(p.exitcode not in (None, 0) for p in ps), [p.exitcode for p in ps]
                assert time.monotonic() - t0 < timeout, "the ranks did not finish"
        for p in ps:
            p.join(timeout=60)
    finally:
        for p in ps:
            if p.is_alive():
                p.kill()
    assert [p.exitcode for p in ps] == [0] * world
    return [r[1] for r in sorted(res, key=lambda t: t[0])]


def deck_par(problem, overrides, blocks):
    """our deck of `problem` with the <outputN> blocks {"N": {key: value}} and the command-line overrides"""
    import re
    text = open(os.path.join(dumpfix.DECKS, "athinput." + problem)).read()
    text = re.sub(r"(?m)^maxout\s*=.*$", "maxout = %d" % max(int(k) for k in blocks), text, count=1)
    for n, kv in sorted(blocks.items(), key=lambda t: int(t[0])):
        text += f"\n<output{n}>\n" + "".join(f"{k} = {v}\n" for k, v in kv.items())
    return pkg("athinput").ParTable.from_text(text).cmdline(list(overrides))


def later_files(full, seed):
    """the files of the uninterrupted run's tree `full` that a run resumed from `seed` (rank 0's file, a path under `full`)
    writes again: of every <outputN> block those from the number the seed's table carries on, and every .hst"""
    import re
    par = pkg("restart").read_head(seed)["par"]
    nxt = {}
    for n in range(1, par.geti("job", "maxout") + 1):
        nxt[par.gets(f"output{n}", "out_fmt")] = par.geti(f"output{n}", "num")
    out = []
    for rel in tree(full):
        m = re.search(r"\.(\d{4})\.(\w+)$", rel)
        if rel.endswith(".hst") or (m and int(m.group(1)) >= nxt[m.group(2)]):
            out.append(rel)
    return out


def compare_resumed_with_full(full, res, seed):
    """every file the resumed run left is the uninterrupted run's, byte for byte (restart dumps too: the parameter text as
    well); a .hst holds the tail of the uninterrupted one and no header"""
    later = later_files(full, seed)
    assert tree(res) == later and len(later) >= 5, (tree(res), later)
    for rel in later:
        a = open(os.path.join(res, rel), "rb").read(); b = open(os.path.join(full, rel), "rb").read()
        if rel.endswith(".hst"):
            rows = a.decode().splitlines()
            assert rows and not any(l.startswith("#") for l in rows), rel
            assert b.decode().splitlines()[-len(rows):] == rows, rel
        else:
            assert a == b, rel
