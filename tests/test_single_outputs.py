"""Single-variable outputs (OutputSet.from_par(single=True); output.c OutData1/2/3, output_vtk.c, output_tab.c, output_pgm.c) on the
host: the slice-index search, the writers fed with the numpy restatement of the payload from the fixtures' states -- byte for byte
against the reference's files (tests/golden/single_*.npz) --, the refusals, and that nothing changes without the keyword."""
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import singlefix                                              # noqa: E402
from singlefix import Fixture, pkg                            # noqa: E402


def _par(text_blocks, nx=(16, 12, 8), deck="blast", maxout=None):
    text = open(os.path.join(singlefix.DECKS, "athinput." + deck)).read()
    import re
    text = re.sub(r"(?ms)^<output\d+>.*?(?=^<|\Z)", "", text)
    text = re.sub(r"(?m)^maxout\s*=.*$", "maxout = %d" % (maxout or len(text_blocks)), text, count=1)
    for n, body in enumerate(text_blocks, 1):
        text += f"\n<output{n}>\n{body}\n"
    return pkg("athinput").ParTable.from_text(text).cmdline([f"domain1/Nx{d + 1}={nx[d]}" for d in range(3)])


# ---- 1. the slice-index search ------------------------------------------------------------------------------------------------
def _brute(l, u, minx, dx, n):
    faces = [minx + float(k) * dx for k in range(n + 1)]
    if u < faces[0] or l >= faces[n]:
        return None
    start = max([k for k in range(1, n + 1) if l >= faces[k]] + [0])       # the zone whose lower face is the last one <= l
    end = max([k for k in range(n) if not u < faces[k]])
    return start, end


@pytest.mark.parametrize("minx,dx,n", [(-0.5, 0.0625, 16), (-0.75, 0.125, 12), (-0.5, 1.0 / 67, 67), (0.0, 0.3, 7)])
def test_slice_search_equals_brute_force(minx, dx, n):
    O = pkg("outputs")
    vals = sorted({minx + k * dx for k in range(n + 1)} | {minx + (k + 0.5) * dx for k in range(-1, n + 1)}
                  | {minx - 1.0, minx + n * dx + 1.0, np.nextafter(minx, -1.0), np.nextafter(minx + n * dx, -1.0)})
    for l in vals:
        for u in vals:
            if l <= u:
                assert O.slice_search(l, u, minx, dx, n) == _brute(l, u, minx, dx, n), (l, u)
    assert O.slice_search(minx, minx, minx, dx, n) == (0, 0)                       # a value on the first face: the first zone
    assert O.slice_search(minx + 3 * dx, minx + 3 * dx, minx, dx, n)[0] in (2, 3)  # (which one: what the face's double says)
    assert O.slice_search(minx - 1.0, minx + n * dx + 1.0, minx, dx, n) == (0, n - 1)
    # the zones the reference SUMS lie nghost above the slice's own (output.c:789-790 adds the first active index twice)
    assert O.slice_zones(minx, minx, minx, dx, n) == (4, 4)
    assert O.slice_zones(minx, minx, minx, dx, 1) == (0, 0)


def test_parse_slice_forms():
    O = pkg("outputs")
    par = _par(["out_fmt = tab\nout = d\ndt = 1\nx1 = 0.25\nx2 = :0.5\nx3 = -0.1:"])
    assert O.parse_slice(par, "output1", "x1", -0.5, 0.5) == (0.25, 0.25, 1)
    assert O.parse_slice(par, "output1", "x2", -0.75, 0.75) == (-0.75, 0.5, 1)
    assert O.parse_slice(par, "output1", "x3", -0.5, 0.5) == (-0.1, 0.5, 1)
    assert O.parse_slice(par, "output2", "x1", -0.5, 0.5) == (-0.5, 0.5, 0)
    with pytest.raises(pkg("athinput").ParError, match="lower slice limit"):
        O.parse_slice(_par(["out_fmt = tab\nout = d\ndt = 1\nx1 = 0.3:0.1"]), "output1", "x1", -0.5, 0.5)


def test_recorded_dimensions():
    """the dimensions the reference's files state are those single_ranges / payload_shape give"""
    O = pkg("outputs")
    for name in singlefix.HYDRO:
        fx = Fixture(name)
        par = fx.par(); run = fx.run_config(par)
        outs = fx.outputs(".", par)
        for o in outs.outs:
            rel = pkg("dumps").fname_id("Blast", 0, 0, 0, o.id, o.out_fmt)
            rng = O.single_ranges(o, run.rootNx, run.xmin, run.dx)
            if rng is None:
                assert rel not in fx.paths
                continue
            shape = O.payload_shape(rng[0], run.rootNx)
            b = fx.file(rel)
            if o.out_fmt == "pgm":
                assert b.startswith(b"P5\n%d %d\n255\n" % (shape[1], shape[0])), (rel, shape)
            elif o.out_fmt == "vtk":
                dims = (shape[-1] + 1, shape[-2] + 1, shape[0] + 1 if len(shape) == 3 else 1)
                assert b"DIMENSIONS %d %d %d\n" % dims in b[:400], (rel, shape)
            else:
                assert b.count(b"\n") == int(np.prod(shape)), (rel, shape)


# ---- 2. the writers, from the fixtures' states ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", singlefix.HYDRO + [singlefix.SPHERE])
def test_host_writers_reproduce_reference_files(name, tmp_path):
    fx = Fixture(name)
    par = fx.par()
    d = singlefix.host_driver(fx, par)
    outs = fx.outputs(tmp_path, par)
    assert outs.single and all(o.single for o in outs.outs) and outs.rst is not None
    for num in fx.nums():
        st, d.time = fx.state(num)
        d.eng.U = fx.block_with_ghosts(num) if "U" in st else None
        d.eng.ef = st.get("ef")
        for o in outs.outs:
            o.num = num
            d.write_single(o, outs)
    singlefix.compare_singles(fx, tmp_path)
    assert all(o.gmin <= o.gmax for o in outs.outs if o.id != "miss")


def test_pgm_quantisation_branches():
    D = pkg("dumps")
    data = np.array([[0.0, 1.0, 2.0], [3.0, 4.0, 5.0]])
    g = D.pgm_gray(data, 0.0, 5.0).reshape(2, 3)
    assert g[0].tolist() == [153, 204, 255] and g[1].tolist() == [0, 51, 102]      # rows from the last to the first; 5.0 stays below 256
    assert D.pgm_gray(data, 2.0, 3.0).reshape(2, 3)[1].tolist() == [0, 0, 0]      # clamped below
    assert D.pgm_gray(data, 2.0, 3.0).reshape(2, 3)[0].tolist() == [255, 255, 255]
    assert not D.pgm_gray(np.full((2, 3), 7.0), 7.0, 7.0).any()                  # max_min == 0
    assert not D.pgm_gray(data, 5.0, 0.0).any()                                  # max_min < 0
    assert D.pgm_gray(np.array([[np.nan, 1e300]]), 0.0, 1.0).tolist() == [0, 0]  # (int) of the host: INT_MIN, clamped to 0
    assert D.minmax(np.array([0.0, -0.0, 1.0]))[0] is not None
    assert np.signbit(D.minmax(np.array([0.0, -0.0, 1.0]))[0]) and not np.signbit(D.minmax(np.array([-0.0, 0.0, 1.0]))[0])


# ---- 3. the numbering: a slice that misses the Grid writes nothing and counts all the same --------------------------------------
def test_missing_slice_advances_the_number(tmp_path):
    fx = Fixture("single_blast_16x12x8_s2")
    par = _par(["out_fmt = pgm\nout = d\nid = miss\ndt = 1e-9\nx3 = 5.0", "out_fmt = tab\nout = d\nid = d\ndt = 1e-9\nx2 = 0.0\nx3 = 0.0\nnum = 7"])
    run = pkg("config").from_par(par, "blast")
    d = pkg("driver").Driver(run, engine_factory=lambda grid: singlefix.HostEngine(fx.block_with_ghosts(0)))
    outs = pkg("outputs").OutputSet.from_par(par, 0.0, str(tmp_path), single=True)
    assert [o.num for o in outs.outs] == [0, 7]                                   # (a restarted run's table continues a block)
    d.data_output(outs, 1); d.data_output(outs, 1)
    assert [o.num for o in outs.outs] == [2, 9]
    assert singlefix.tree(tmp_path) == ["Blast.0007.d.tab", "Blast.0008.d.tab"]


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("body,match", [
    ("out_fmt = ppm\nout = d\ndt = 1", "ppm.*palette"),
    ("out_fmt = pdf\nout = d\ndt = 1", "pdf"),
    ("name = foo\nout_fmt = vtk\ndt = 1", "name = foo"),
    ("out_fmt = vtk\nout = S\ndt = 1", "out = S.*pow"),
    ("out_fmt = vtk\nout = dpar\ndt = 1", "dpar.*particle"),
    ("out_fmt = tab\nout = cons\ndt = 1", "out_fmt=tab for out=cons"),
    ("out_fmt = tab\nout = prim\ndt = 1", "out_fmt=tab for out=prim"),
    ("out_fmt = vtk\nout = B1c\ndt = 1", "B1c.*Unknown data expression"),
    ("out_fmt = vtk\nout = flux\ndt = 1", "flux.*Unknown data expression"),     # without usr_expr_flag getexpr does not know it
    ("out_fmt = vtk\nout = d\nusr_expr_flag = 1\ndt = 1", "user expression"),
    ("out_fmt = bin\nout = d\ndt = 1", "out_fmt=bin"),
    ("out_fmt = tab\nout = d\ndt = 1\nx1 = 0\nx2 = 0\nx3 = 0", "Too many slices"),
    ("out_fmt = vtk\nout = d\ndt = 1\nx1 = 0\nx2 = 0", "Only able to output 2D or 3D"),
    ("out_fmt = pgm\nout = d\ndt = 1", "2D slice"),
])
def test_refused_under_the_keyword(body, match):
    with pytest.raises(pkg("athinput").ParError, match=match):
        pkg("outputs").OutputSet.from_par(_par([body]), 0.0, ".", single=True)


def test_keyword_refusals_of_runs():
    O = pkg("outputs")
    body = "out_fmt = vtk\nout = d\ndt = 1"
    with pytest.raises(ValueError, match="one-rank"):
        O.OutputSet.from_par(_par([body]), 0.0, ".", rank=0, nranks=2, single=True)
    with pytest.raises(ValueError, match="1-D Grid"):
        O.OutputSet.from_par(_par([body], nx=(16, 1, 1)), 0.0, ".", single=True)
    with pytest.raises(ValueError, match="overlap"):
        O.OutputSet.from_par(_par([body]), 0.0, ".", single=True, overlap=True)
    with pytest.raises(pkg("athinput").ParError, match="defines no such expression"):
        O.OutputSet.from_par(_par(["out_fmt = vtk\nout = flux\nusr_expr_flag = 1\ndt = 1"]), 0.0, ".", single=True, problem="blast")
    outs = O.OutputSet.from_par(_par([body]), 0.0, ".", single=True)
    D = pkg("driver")
    for cls, word in ((D.MeshRun, "MeshRun"), (D.MeshDriver, "MeshDriver")):
        t = cls.__new__(cls)                      # (asked before anything of the run is read)
        with pytest.raises(ValueError, match=word):
            outs.data_output(t, 1)
    # a problem without the expression is refused before the first file
    fx = Fixture("single_blast_16x12x8_s2")
    par = _par(["out_fmt = vtk\nout = flux\nusr_expr_flag = 1\ndt = 1"])
    d = D.Driver(pkg("config").from_par(par, "blast"), engine_factory=lambda grid: singlefix.HostEngine(fx.block_with_ghosts(0)))
    with pytest.raises(ValueError, match="defines no such expression"):
        d.data_output(O.OutputSet.from_par(par, 0.0, ".", single=True), 1)


def test_without_the_keyword_nothing_changes():
    O = pkg("outputs"); E = pkg("athinput").ParError
    assert inspect.signature(O.OutputSet.from_par).parameters["single"].default is False
    with pytest.raises(E) as e:
        O.OutputSet.from_par(_par(["out_fmt = vtk\nout = d\ndt = 1"]), 0.0, ".")
    assert str(e.value) == ("[init_output]: <output1> out = d (out_fmt = vtk): single-variable outputs are not built; "
                            "dumps take out = cons or out = prim")
    with pytest.raises(E, match="Unsupported dump mode for output1/out_fmt=ppm for out=cons"):
        O.OutputSet.from_par(_par(["out_fmt = ppm\ndt = 1"]), 0.0, ".")
    outs = O.OutputSet.from_par(_par(["out_fmt = vtk\ndt = 1", "out_fmt = hst\ndt = 1"]), 0.0, ".")
    assert not outs.single and not any(o.single for o in outs.outs)


def test_shipped_deck_reads():
    par = pkg("athinput").ParTable.from_file(os.path.join(singlefix.DECKS, "athinput.blast_single")) \
        if hasattr(pkg("athinput").ParTable, "from_file") else \
        pkg("athinput").ParTable.from_text(open(os.path.join(singlefix.DECKS, "athinput.blast_single")).read())
    outs = pkg("outputs").OutputSet.from_par(par, 0.0, ".", single=True)
    assert {o.out_fmt for o in outs.outs} >= {"hst", "vtk", "tab", "pgm"} and any(o.single for o in outs.outs)
    with pytest.raises(pkg("athinput").ParError, match="single-variable outputs are not built"):
        pkg("outputs").OutputSet.from_par(par, 0.0, ".")
