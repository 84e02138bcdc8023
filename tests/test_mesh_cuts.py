"""csrc/mesh_cuts.h -- the cut arithmetic of a Mesh on in-library slabs, plain C without a device -- against config.mesh_slabs:
spans, the links in the layout aa_mesh_create_local takes, corr_to and corr_in of every slab, over the random nestings and cuts
of test_distributed_smr_gloo.py::test_mesh_slab_invariants_random (same generator, same seed, 60 accepted meshes) and the seven
parameter sets of test_gpu_smr_slabs.py.  Where mesh_slabs refuses (a thin piece, bad cuts) the C side must refuse too."""
import ctypes as C
import importlib
import os
import random
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
PKG = os.path.join(os.path.dirname(HERE), "atmospheric-athena_amd")
DECKS = os.path.join(PKG, "decks")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("mesh_cuts") / "mesh_cuts_probe.so")
    subprocess.check_call(["gcc", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(PKG, "csrc"),
                           os.path.join(HERE, "fixtures", "mesh_cuts_probe.c"), "-o", so])
    L = C.CDLL(so)
    ip = C.POINTER(C.c_int)
    L.probe_mesh_cuts.restype = C.c_int
    L.probe_mesh_cuts.argtypes = [C.c_int, ip, ip, ip, C.c_int, ip, C.c_int, ip, C.c_int, C.c_char_p, C.c_int]
    return L


def c_side(L, levs, run, nslab, cuts):
    """-> (per slab: spans, links, corr_in) or the error message"""
    ints = lambda v: (C.c_int * len(v))(*v)
    nx = [g.Nx[d] for g in levs for d in range(3)]
    disp = [g.disp[d] if g.level else 0 for g in levs for d in range(3)]
    out = (C.c_int * 65536)()
    err = C.create_string_buffer(512)
    periodic3 = int(run.bc[4] == 4 and run.bc[5] == 4)
    n = L.probe_mesh_cuts(len(levs), ints(nx), ints(disp), ints(list(run.rootNx)), nslab, ints(list(cuts)) if cuts is not None else None,
                          periodic3, out, len(out), err, len(err))
    if n < 0:
        return err.value.decode()
    w = list(out[:n]); pos = 0
    slabs = []
    for _ in range(nslab):
        nl = w[pos]; pos += 1
        spans = [tuple(w[pos + 4 * l:pos + 4 * l + 4]) for l in range(nl)]; pos += 4 * nl
        links = [tuple(w[pos + 23 * l:pos + 23 * l + 23]) for l in range(max(nl - 1, 0))]; pos += 23 * max(nl - 1, 0)
        nc = w[pos]; pos += 1
        corr_in = [tuple(w[pos + 7 * q:pos + 7 * q + 7]) for q in range(nc)]; pos += 7 * nc
        slabs.append((spans, links, corr_in))
    assert pos == n
    return slabs


def compare(L, aa, par, run, levs, nslab, cuts):
    """config.mesh_slabs and the header agree on every slab, or both refuse; -> whether the mesh was accepted"""
    try:
        cfgs = [aa.config.mesh_slabs(par, run, r, nslab, cuts) for r in range(nslab)]
    except aa.athinput.ParError:
        cfgs = None
    ccuts = cuts if cuts is not None else aa.config.balanced_cuts(levs, nslab)
    got = c_side(L, levs, run, nslab, ccuts)
    if cfgs is None:
        assert isinstance(got, str) and got, "mesh_slabs refuses these cuts: the C side must report an error too"
        return False
    assert not isinstance(got, str), got
    for c, (spans, links, corr_in) in zip(cfgs, got):
        assert len(spans) == len(c.levels)
        for l, g in enumerate(c.levels):
            assert spans[l][:2] == c.table[c.rank][l]
            assert spans[l][2:] == (g.lx3, g.rx3)
            assert g.bc[4] == (0 if g.lx3 >= 0 else levs[l].bc[4]) and g.bc[5] == (0 if g.rx3 >= 0 else levs[l].bc[5])
        for l in range(len(c.levels), len(levs)):
            assert c.table[c.rank][l] is None
        assert len(links) == len(c.links)
        for mine, K in zip(links, c.links):
            assert mine == (*K.cs, *K.n, *K.prol, *K.corr, *K.cdisp, *K.corr_to)
        assert corr_in == [tuple(q) for q in c.corr_in]
    return True


def dom(n, nx, disp=None):
    o = [f"domain{n}/Nx{d + 1}={nx[d]}" for d in range(3)]
    if disp:
        o += [f"domain{n}/{k}Disp={disp[d]}" for d, k in enumerate("ijk")]
    return o


def test_random_nestings(probe):
    aa = importlib.import_module("atmospheric-athena_amd")
    rng = random.Random(7)
    tried = refused = 0
    while tried < 60:
        n3 = rng.choice([16, 24, 32, 40])
        nlev = rng.choice([2, 3])
        ov = [f"job/num_domains={nlev}"] + dom(1, (8, 8, n3))
        lo, hi = 0, n3
        ok = True
        for l in range(1, nlev):
            a = rng.randrange(lo // 1 + 2, (lo + hi) // 2, 2) if rng.random() < 0.8 or lo != 0 else 0
            b = rng.randrange((lo + hi) // 2 + 2, hi - 1, 2)
            if b - a < 4:
                ok = False; break
            ov += dom(l + 1, (8, 8, 2 * (b - a)), (4 * (2 ** (l - 1)) if l == 1 else 0, 0, 2 * a))
            lo, hi = 2 * a, 2 * b
        if not ok:
            continue
        ov = [o for o in ov if not o.startswith("domain") or "Disp" not in o or o.split("/")[1][0] == "k"] + \
             ["domain1/bc_ix1=2", "domain1/bc_ox1=2", "domain1/bc_ix2=2", "domain1/bc_ox2=2", "domain1/bc_ix3=2", "domain1/bc_ox3=2"]
        for l in range(1, nlev):
            ov += [f"domain{l + 1}/iDisp=0", f"domain{l + 1}/jDisp=0", f"domain{l + 1}/Nx1={8 * 2 ** l}", f"domain{l + 1}/Nx2={8 * 2 ** l}"]
        try:
            par = aa.athinput.ParTable.from_file(os.path.join(DECKS, "athinput.blast")).cmdline(ov)
            run = aa.config.from_par(par, "blast")
            levs = aa.config.levels(par, run)
        except aa.athinput.ParError:
            continue
        nranks = rng.choice([2, 3, 4])
        cuts = None
        if rng.random() < 0.5:
            g1 = levs[1]
            cand = sorted({0, g1.disp[2] // 2, (g1.disp[2] + g1.Nx[2]) // 2, n3})
            if all(b - a >= 4 for a, b in zip(cand, cand[1:])):
                cuts, nranks = tuple(cand), len(cand) - 1
        if compare(probe, aa, par, run, levs, nranks, cuts):
            tried += 1
        else:
            refused += 1
    assert refused > 0, "the generator is known to produce thin pieces: the refusals must have been compared too"


def _smr_slab_sets():
    import test_gpu_smr_slabs as t
    (mark,) = [m for m in t.test_two_slab_stacks_equal_one_mesh.pytestmark if m.name == "parametrize"]
    return [p[:3] for p in mark.args[1]]


@pytest.mark.parametrize("case", range(7))
def test_smr_slab_parameter_sets(probe, case):
    aa = importlib.import_module("atmospheric-athena_amd")
    sets = _smr_slab_sets()
    assert len(sets) == 7
    problem, overrides, cuts = sets[case]
    par = aa.athinput.ParTable.from_file(os.path.join(DECKS, "athinput." + problem)).cmdline(overrides)
    run = aa.config.from_par(par, problem)
    assert compare(probe, aa, par, run, aa.config.levels(par, run), 2, cuts)


def test_equal_division_and_periodic_root(probe):
    """cuts == NULL is the root's equal division of slabs_create (Nx3/N planes, the remainder to the first slabs); a periodic
    root wraps on the root level only; a piece thinner than nghost names the level, the slab and the cut"""
    aa = importlib.import_module("atmospheric-athena_amd")
    ov = ["job/num_domains=2"] + dom(1, (16, 16, 26)) + dom(2, (16, 16, 24), (8, 8, 12))
    par = aa.athinput.ParTable.from_file(os.path.join(DECKS, "athinput.blast")).cmdline(ov)
    run = aa.config.from_par(par, "blast")
    levs = aa.config.levels(par, run)
    got = c_side(probe, levs, run, 3, None)
    assert [s[0][0][:2] for s in got] == [(0, 9), (9, 18), (18, 26)]
    assert compare(probe, aa, par, run, levs, 3, (0, 9, 18, 26))
    periodic = run.bc[4] == 4 and run.bc[5] == 4
    assert (got[0][0][0][2], got[2][0][0][3]) == ((2, 0) if periodic else (-1, -1))
    assert all(p[2] in (-1, s - 1) and p[3] in (-1, s + 1) for s, sl in enumerate(got) for p in sl[0][1:])
    assert [len(s[0]) for s in got] == [2, 2, 1], "slab 2 holds no zones of level 1"
    msg = c_side(probe, levs, run, 2, (0, 7, 26))         # level 1 = planes 12 .. 36: 2 planes below root plane 7
    assert isinstance(msg, str) and "level 1" in msg and "slab 0" in msg and "plane 7" in msg
    assert not compare(probe, aa, par, run, levs, 2, (0, 7, 26))
