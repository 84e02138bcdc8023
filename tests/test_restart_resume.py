"""Continuing a run from a restart dump (``athena -r file.rst [block/key=value ...]``), on the CPU.

Fixtures: tests/golden/restart_*.npz -- runs of the UNMODIFIED reference executables that were interrupted and continued with -r
(tests/golden/make_golden_restart.py); every fixture holds the seed file(s) and the tree the RESUMED run left.  The Driver runs on
the oracle engine (bit for bit on blast), so what is tested is the reader, the table with its overrides, the start sequence of a
restarted run (no new_dt, no forced first output), the continued numbering, the .hst without a second header and the N-rank
naming rules."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import dumpfix                                         # noqa: E402
import restartfix                                      # noqa: E402
from dumpfix import pkg                                # noqa: E402
from restartfix import RFixture                        # noqa: E402
from test_distributed_gloo import OracleEngine, _free_port     # noqa: E402


class RestartOracleEngine(OracleEngine):
    """OracleEngine that takes the state of a restart dump (the optional engine method load_state) and adds up the history sums
    zone by zone in the reference's order (dump_history.c:171-202), so that the columns that are round-off noise agree too."""

    def load_state(self, U_active, edgeflux):
        self.s.active[..., :U_active.shape[-1]] = U_active
        if edgeflux is not None:
            self.s.edgeflux[...] = edgeflux

    def download_edgeflux(self):
        return self.s.edgeflux.copy()

    def history(self):
        dx = self.cfg.run.dx
        dVol = 1.0
        for d in range(3):
            dVol *= dx[d]
        U = self.s.active.reshape(-1, 6)
        d, M1, M2, M3, E = (U[:, c] for c in range(5))
        d1 = 1.0 / d
        terms = [dVol * d, dVol * E, dVol * M1, dVol * M2, dVol * M3,
                 dVol * 0.5 * (M1 * M1) * d1, dVol * 0.5 * (M2 * M2) * d1, dVol * 0.5 * (M3 * M3) * d1,
                 dVol * U[:, 5] if self.cfg.run.nscal else 0.0 * d]
        return np.array([np.cumsum(t)[-1] for t in terms])       # (cumsum adds in order, one zone after the other)


# ---- 1. the reader against every seed ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", restartfix.FIXTURES)
def test_reader_against_the_reference_seeds(name, tmp_path):
    R = pkg("restart"); A = pkg("athinput")
    fx = RFixture(name)
    rank0 = fx.write_seeds(str(tmp_path))
    for rank in range(fx.nranks):
        p = R.rank_path(rank0, rank)
        nxs = fx.level_nx(rank)
        r = R.scan_rst(p, nxs, fx.nscal, fx.ion)
        # the same values as the readers the fixtures were made with
        if fx.levels:
            ref = R.read_rst_levels(p, nxs, fx.nscal, fx.ion)
            ref_levels = ref["levels"]
        else:
            ref = R.read_rst(p, nxs[0], fx.nscal, fx.ion)
            ref_levels = [(ref["U"], ref["edgeflux"])]
        assert (r["nstep"], r["time"], r["dt"]) == (ref["nstep"], ref["time"], ref["dt"]) == (fx.seed_nstep, fx.seed_time, fx.seed_dt)
        for l, nx in enumerate(nxs):
            U, ef = R.read_state(r, l, nx, fx.nscal)
            assert np.array_equal(U.view(np.uint64), ref_levels[l][0].view(np.uint64))
            assert (ef is None) == (not fx.ion) and (ef is None or np.array_equal(ef, ref_levels[l][1]))
        # the offsets add up to the file size: header, labels, payload, USER_DATA and nothing behind it
        last = r["levels"][-1][-1]
        assert last[1] + 8 * last[2] + len(b"\nUSER_DATA\n") == os.path.getsize(p) == r["size"]
        pos = r["offset"]
        for secs in r["levels"]:
            for label, off, n in secs:
                assert off == pos + len(label) + 2
                pos = off + 8 * n
        # the header: comments are dropped, the <comment> / <configure>-style blocks parse, the <outputN> blocks carry num / time
        par = r["par"]
        assert par.gets("job", "problem_id").lower() == fx.problem + ("-id%d" % rank if rank else "") and "comment" in par.blocks
        assert "#" not in par.gets("job", "problem_id")
        assert par.geti("output1", "num") >= 1 and par.getd("output1", "time") > 0
        assert par.geti("time", "nstep") == fx.seed_nstep
    # overrides: an existing key changes, an unknown one is an error (par_cmdline)
    par = R.read_head(rank0)["par"]
    assert par.cmdline(["time/nlim=11"]).geti("time", "nlim") == 11
    with pytest.raises(A.ParError):
        par.cmdline(["time/no_such_key=1"])
    with pytest.raises(A.ParError):
        par.cmdline(["no_such_block/nlim=1"])
    # a truncated copy, a copy with bytes behind USER_DATA and a file read for another mesh are refused with the reference's message
    b = fx.seed_bytes(fx.seed_names.index([s for s in fx.seed_names if "-id" not in s][0]))
    for what, data in (("cut", b[:len(b) - 4000]), ("short", b[:len(b) - 3]), ("long", b + b"12345678")):
        q = str(tmp_path / (what + ".rst"))
        open(q, "wb").write(data)
        with pytest.raises(R.RestartError, match=r"\[restart_grids\]: Expected "):
            R.scan_rst(q, fx.level_nx(0), fx.nscal, fx.ion)
    with pytest.raises(R.RestartError, match=r"\[restart_grids\]: Expected "):
        nx = fx.level_nx(0)
        R.scan_rst(rank0, [(nx[0][0] + 1, nx[0][1], nx[0][2])] + nx[1:], fx.nscal, fx.ion)


# ---- 2. the Driver on the oracle engine, resumed from the reference's seed ------------------------------------------
@pytest.mark.parametrize("name", ["restart_blast_16x12x8_s3_s8", "restart_blast_16x12x8_s3_s11"])
def test_resumed_driver_leaves_the_reference_resumed_tree(name, tmp_path):
    fx = RFixture(name)
    seed = fx.write_seeds(str(tmp_path / "seed"))
    d = pkg("driver").Driver.from_restart(seed, fx.resume_overrides, engine_factory=RestartOracleEngine)
    assert d.restarted and d.nstep == fx.seed_nstep
    t0, dt0 = d.time, d.dt
    rundir = str(tmp_path / "run")
    outs = pkg("outputs").OutputSet.from_par(d.par, d.time, rundir)
    d.start()
    assert (d.time, d.dt, d.nstep) == (t0, dt0, fx.seed_nstep)          # no new_dt: the file's dt is the next step's
    d.main(outs)
    assert d.nstep == fx.nlim                                            # (_s11: time/nlim=11 from the command line)
    restartfix.compare_resumed_tree(fx, rundir)
    first = min(fx.where(p)[2] for p in fx.paths if not p.endswith(".hst"))
    assert first == 2 and not os.path.exists(os.path.join(rundir, "Blast.0001.vtk"))      # no forced first output
    assert not open(os.path.join(rundir, "Blast.hst")).read().startswith("#")


# ---- 3. two ranks under gloo ------------------------------------------------------------------------------------------
def _rank_main(rank, world, port, name, seed, rundir, q):
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    fx = RFixture(name)
    d = pkg("driver").Driver.from_restart(seed, fx.resume_overrides, engine_factory=RestartOracleEngine, rank=rank, nranks=world)
    outs = pkg("outputs").OutputSet.from_par(d.par, d.time, rundir, rank, world)
    d.main(outs)
    q.put((rank, d.nstep, outs.basename))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("by_rank", [False, True])
def test_two_ranks_resume_from_their_own_files(by_rank, tmp_path):
    """both seed files in one directory (where the reference looks), and laid out as the ranks wrote them (id0/, id1/)"""
    import torch.multiprocessing as mp
    name = "restart_blast_mpi2_16x12x8_s3_s8"
    fx = RFixture(name)
    seed = fx.write_seeds(str(tmp_path / "seed"), by_rank=by_rank)
    rundir = str(tmp_path / "run")
    ctx = mp.get_context("spawn")
    q = ctx.Queue(); port = _free_port()
    ps = [ctx.Process(target=_rank_main, args=(r, 2, port, name, seed, rundir, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = sorted(q.get(timeout=300) for _ in range(2))
    for p in ps:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res == [(0, fx.nlim, "Blast"), (1, fx.nlim, "Blast-id1")]      # rank 1: Blast-id1.*, not Blast-id1-id1.*
    restartfix.compare_resumed_tree(fx, rundir)


# ---- 4. our own files: resumed equals uninterrupted ------------------------------------------------------------------
def test_resumed_from_our_own_file_equals_the_uninterrupted_run(tmp_path):
    fx = RFixture("restart_blast_16x12x8_s3_s8")
    par = fx.par(); run = fx.run_config(par)
    full = str(tmp_path / "full"); res = str(tmp_path / "resumed")
    d = pkg("driver").Driver(run, RestartOracleEngine)
    d.main(pkg("outputs").OutputSet.from_par(par, 0.0, full))
    assert d.nstep == fx.nlim
    seed = os.path.join(full, "Blast.0001.rst")
    r = pkg("driver").Driver.from_restart(seed, engine_factory=RestartOracleEngine)
    assert 0 < r.nstep < fx.nlim
    r.main(pkg("outputs").OutputSet.from_par(r.par, r.time, res))
    assert (r.time, r.dt, r.nstep) == (d.time, d.dt, d.nstep)
    assert np.array_equal(r.eng.download(), d.eng.download())
    later = [p for p in restartfix.tree(full) if p.endswith(".hst") or fx.where(p)[2] > 1]
    assert restartfix.tree(res) == later and len(later) >= 5
    for rel in later:
        a = open(os.path.join(res, rel), "rb").read(); b = open(os.path.join(full, rel), "rb").read()
        if rel.endswith(".hst"):
            rows = a.decode().splitlines()
            assert rows and not any(l.startswith("#") for l in rows)
            assert b.decode().splitlines()[-len(rows):] == rows          # the tail of the uninterrupted file, and no header
        else:
            assert a == b, rel                                           # restart dumps too: the parameter text as well


# ---- 5. the defaults are unchanged ------------------------------------------------------------------------------------
def test_history_writer_and_outputs_run_defaults(tmp_path):
    hist = pkg("history"); O = pkg("outputs")
    w = hist.HistoryWriter(str(tmp_path), "X")
    w.dump(0.0, 0.1, np.arange(9.0), 2.0, 0)
    w.dump(0.1, 0.1, np.arange(9.0), 2.0, 0)
    lines = open(w.path).read().splitlines()
    assert [l.startswith("#") for l in lines] == [True, True, True, False, False]
    w = hist.HistoryWriter(str(tmp_path), "Y", num=3)                    # the block's num of a resumed run: rows, no header
    w.dump(0.0, 0.1, np.arange(9.0), 2.0, 0)
    assert not open(w.path).read().startswith("#")

    class Target:
        def __init__(self, restarted=None):
            self.time, self.nstep, self.calls = 0.0, 0, []
            if restarted is not None:
                self.restarted = restarted

        def start(self): self.calls.append("start")
        def step(self): self.nstep += 1; self.time += 1.0

    class Outs:
        def data_output(self, target, flag): target.calls.append(("out", flag, target.nstep))

    for restarted, want in ((None, True), (False, True), (True, False)):
        t = Target(restarted)
        O.run(t, Outs(), 10.0, 2)
        forced_first = t.calls[:2] == ["start", ("out", 1, 0)]
        assert forced_first == want, (restarted, t.calls)
        assert t.calls[-1] == ("out", 1, 2) and t.calls.count(("out", 0, 0)) == 1
