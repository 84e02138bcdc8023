"""The reference's vtk / bin data dumps and its <outputN> machinery, on the CPU.

Fixtures: tests/golden/dump_*.npz -- the files the UNMODIFIED reference executables wrote (tests/golden/make_golden_dumps.py),
with the state of every dump instant read from the restart dump written beside it.  Rule for every dump file: byte for byte,
headers included, except that a word that is NaN in the reference's file only has to be NaN in ours; the fixture may hold such
words in at most 0.1 % of a file (dumpfix.compare_dump counts them from the fixture).
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import dumpfix                     # noqa: E402
from dumpfix import Fixture, pkg    # noqa: E402


# ---- 1. payload_from_block + the writers against every file of every fixture ----------------------------------
@pytest.mark.parametrize("name", dumpfix.FIXTURES)
def test_host_payload_and_writers_reproduce_reference_files(name, tmp_path):
    fx = Fixture(name)
    files = fx.dumps()
    assert files
    nan_total = 0
    for rel in files:
        p = str(tmp_path / "f")
        g = dumpfix.write_from_block(p, fx, rel)
        ext = rel.rsplit(".", 1)[1]
        nan_total += dumpfix.compare_dump(open(p, "rb").read(), fx.file(rel), g.Nx, fx.nscal, ext, fx.prim_of(ext), f"{name}:{rel}")
    print(f"{name}: {len(files)} files equal, {nan_total} NaN words in the reference's files")


def test_fixtures_cover_the_cases():
    """what the fixtures are there for: both formats with both variable sets, a scalar, NaN and negative pressures, an odd Nx1,
    two ranks, a refined level, a cadence that skips passes"""
    seen = set()
    for name in dumpfix.FIXTURES:
        fx = Fixture(name)
        for rel in fx.dumps():
            ext = rel.rsplit(".", 1)[1]
            seen.add((ext, fx.prim_of(ext)))
    assert seen == {("vtk", False), ("vtk", True), ("bin", False), ("bin", True)}
    assert Fixture("dump_blast_13x6x5_s3_vtkprim").nx[0] % 2 == 1
    fx = Fixture("dump_ioniz_sphere_20x20x20_s3")
    U, _t, _dt = fx.state("ioniz_sphere.0003.vtk")
    with np.errstate(all="ignore"):
        P = (U[..., 4] - 0.5 * (U[..., 1] ** 2 + U[..., 2] ** 2 + U[..., 3] ** 2) / U[..., 0])
    assert np.isnan(P).any() and (P < 0).any()
    fx = Fixture("dump_blast_cadence_16x12x8_s8")
    i = fx.rst_index(0, max(fx.where(p)[2] for p in fx.paths))
    assert int(fx.z[f"rst_{i}_nstep"]) == 8 and fx.where(fx.paths[i])[2] < 8        # `num` and the step count part ways
    assert any(p.startswith("id1/") for p in Fixture("dump_blast_mpi2_16x12x8_s2").paths)
    assert any(p.startswith("lev1/") for p in Fixture("dump_blast_smr_16x12x8_s1").paths)


def test_nan_pressure_becomes_tiny_number():
    """the reference's MAX(P, TINY_NUMBER) sends a NaN pressure to TINY_NUMBER; density NaN stays NaN"""
    D = pkg("dumps")
    U = np.ones((1, 1, 4, 5)); U[0, 0, :, 4] = [np.nan, -1.0, 0.0, 10.0]
    pay = D.payload_from_block(U, "bin", True, 1.5)
    assert pay[4].tolist() == [np.float32(1e-20)] * 3 + [4.25]


# ---- 2. OutputSet + Driver on the oracle engine: the whole tree of the blast runs ---------------------------------
@pytest.mark.parametrize("name", ["dump_blast_16x12x8_s5", "dump_blast_13x6x5_s3_vtkprim", "dump_blast_13x6x5_s3_bincons",
                                  "dump_blast_cadence_16x12x8_s8"])
def test_driver_on_oracle_engine_leaves_the_reference_tree(name, tmp_path):
    from test_distributed_gloo import OracleEngine
    fx = Fixture(name)
    par = fx.par(); run = fx.run_config(par)
    d = pkg("driver").Driver(run, OracleEngine)
    outs = pkg("outputs").OutputSet.from_par(par, 0.0, str(tmp_path))
    d.main(outs)
    assert d.nstep == fx.nlim
    dumpfix.compare_tree(fx, str(tmp_path))
    assert sorted(set(outs.written)) == fx.paths          # (two vtk blocks write the same names: the later one stays)


# ---- 3. two ranks under gloo: id0/, id1/ ---------------------------------------------------------------------------
def _rank_main(rank, world, port, name, rundir, q):
    import torch.distributed as dist
    from test_distributed_gloo import OracleEngine
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    fx = Fixture(name)
    par = fx.par(); run = fx.run_config(par)
    d = pkg("driver").Driver(run, OracleEngine, rank, world)
    outs = pkg("outputs").OutputSet.from_par(par, 0.0, rundir, rank, world)
    d.main(outs)
    q.put((rank, d.nstep, sorted(outs.written)))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_write_their_own_grids(tmp_path):
    import torch.multiprocessing as mp
    from test_distributed_gloo import _free_port
    name = "dump_blast_mpi2_16x12x8_s2"
    fx = Fixture(name)
    ctx = mp.get_context("spawn")
    q = ctx.Queue(); port = _free_port()
    ps = [ctx.Process(target=_rank_main, args=(r, 2, port, name, str(tmp_path), q)) for r in range(2)]
    for p in ps:
        p.start()
    res = sorted(q.get(timeout=300) for _ in range(2))
    for p in ps:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert [r[1] for r in res] == [fx.nlim, fx.nlim]
    dumpfix.compare_tree(fx, str(tmp_path))
    # rank 1 writes its own Grid: DIMENSIONS 17 13 5 and the ORIGIN of its slab
    head = open(tmp_path / "id1" / "Blast-id1.0000.vtk", "rb").read(300)
    assert b"DIMENSIONS 17 13 5\n" in head and b"ORIGIN -5.000000e-01 -7.500000e-01 0.000000e+00 \n" in head


# ---- 4. what is not built is refused when the deck is read -----------------------------------------------------------
@pytest.mark.parametrize("kv,words", [
    ({"out_fmt": "ppm", "dt": "0.1"}, ("output2", "ppm")),
    ({"out_fmt": "vtk", "out": "d", "dt": "0.1"}, ("output2", "out = d")),
    ({"name": "my_output", "dt": "0.1"}, ("output2", "my_output")),
    ({"out_fmt": "tab", "out": "prim", "dt": "0.1"}, ("output2", "tab")),
    ({"out_fmt": "hst", "out": "prim", "dt": "0.1"}, ("output2", "hst")),
])
def test_from_par_refuses_what_is_not_built(kv, words):
    fx = Fixture("dump_blast_16x12x8_s5")
    fx.blocks = {"1": {"out_fmt": "rst", "dt": "1.0"}, "2": kv}
    with pytest.raises(pkg("athinput").ParError) as e:
        pkg("outputs").OutputSet.from_par(fx.par(), 0.0)
    for w in words:
        assert w in str(e.value), str(e.value)


def test_from_par_reads_the_keys_and_continues_a_numbering():
    fx = Fixture("dump_blast_16x12x8_s5")
    fx.blocks = {"1": {"out_fmt": "rst", "dt": "1.0"}, "2": {"out_fmt": "bin", "dt": "0.5", "num": "7", "time": "0.25", "level": "1"},
                 "3": {"out_fmt": "hst", "dt": "0.1"}}
    o = pkg("outputs").OutputSet.from_par(fx.par(), 0.125)
    assert o.rst.n == 1 and [x.n for x in o.outs] == [2, 3]
    b = o.outs[0]
    assert (b.out_fmt, b.out, b.num, b.t, b.dt, b.level, b.domain) == ("bin", "cons", 7, 0.25, 0.5, 1, -1)
    assert o.outs[1].t == 0.125 and o.outs[1].num == 0          # `time` defaults to the current time


def test_file_names():
    f = pkg("dumps").fname
    assert f("Blast", 0, 0, 3, "vtk") == "Blast.0003.vtk"
    assert f("Blast", 1, 0, 12, "bin") == os.path.join("lev1", "Blast-lev1.0012.bin")
    assert f("Blast-id2", 2, 1, 0, "vtk") == os.path.join("lev2", "Blast-id2-lev2-dom1.0000.vtk")


def test_shipped_output_deck_has_the_reference_blocks():
    """decks/athinput.ioniz_sphere_out = the headline deck with the two <outputN> blocks the reference ships for it"""
    par = pkg("athinput").ParTable.from_file(os.path.join(dumpfix.DECKS, "athinput.ioniz_sphere_out"))
    run = pkg("config").from_par(par, "ioniz_sphere")
    base = pkg("config").load(os.path.join(dumpfix.DECKS, "athinput.ioniz_sphere"), None, "ioniz_sphere")
    assert run == base                                   # the same run; only the outputs are added
    o = pkg("outputs").OutputSet.from_par(par, 0.0)
    assert (o.rst.out_fmt, o.rst.dt) == ("rst", 1e4)
    assert [(x.out_fmt, x.out, x.dt, x.level, x.domain) for x in o.outs] == [("vtk", "prim", 5e3, -1, -1)]
    assert o.basename == "ioniz_sphere"
