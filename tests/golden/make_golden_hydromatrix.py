#!/usr/bin/env python3
"""Golden fixtures of the designed hydro state (tests/hydromatrix.py, tests/fixtures/hydro_matrix.c), from the REAL reference.

Runs only where the reference lies (like make_golden.py).  `make -f Makefile.ref hydromatrix hydromatrix_cov` links our problem
file into the objects of the hydro-only configurations (blast, blast_noh, blast_vl, blast_ppm, blast_vl_ppm, blast_smr,
blast_smr_vl) in place of prob/blast.c, once as they are and once compiled with gcc --coverage at the same optimisation level.

    tests/golden/hydromatrix_<cfg>_<nx>_n3.npz        single level, 3-D (24x20x16, 67x10x9) and 2-D (67x35, 24x20; Nx3 = 1 picks the
                                                      2-D integrators): nx, U0, U [k][j][i][5], nstep, time, dt, dt0, overrides (for OUR
                                                      deck decks/athinput.blast), cfg, dvac, pvac, cov_roe
    tests/golden/hydromatrix_smr_<3d|2d>_<ctu|vl>_n3.npz  nested levels: nlevels, nxs, levels, disp, U0_<l>, U_<l>, the same scalars, and
                                                      ref_twin_spread / ref_twin_nflip: how far the reference's own six 1-ulp twins of
                                                      the run (the problem file's `seed` key) part from it, |a - b| over each field's
                                                      maximum, and the most zones beyond 1e-9

    tests/golden/hydromatrix_s1_<cfg>_<nx>_n3.npz     the same runs with a passive scalar (`make -f Makefile.ref hydromatrix_scal
    tests/golden/hydromatrix_s1_smr_3d_ctu_n3.npz     hydromatrix_scal_cov`: the NSCALARS = 1 configurations sphere_hydro*, no ion radiation), 3-D only:
                                                      s0, s [k][j][i] (s0_<l>, s_<l> per level), the sixth column before and after; base, the name
                                                      of the scalar-free fixture of the same run; conc_range, the least and the largest
                                                      concentration s / d after the run; the nested one also the reference's own twins of
                                                      the six-variable run.  The scalar is passive: this script ASSERTS that the reference's
                                                      hydro columns, dt0, dt, time and cov_roe of the scalar run equal the base fixture's bit
                                                      for bit and logs it per configuration; the five columns are therefore not stored twice
                                                      (tests/hydromatrix.py `load` puts the two files together).  A configuration in which that
                                                      did not hold would be stored whole (U0, U of six columns, nscal = 1, no base): none is.

`check` regenerates hydromatrix_ctu_67x10x9_n3 from the problem file as it stands and asserts every array of it equal, byte for byte,
to the committed file's (the archive itself carries the time of writing): NSCALARS = 0 compiles to the same behaviour.

cov_roe [step][4]: how often the run took the F = Fl return (roe.c:216), the F = Fr return (:227), the HLLE fallback by
u_inter[0] <= 0 (the tests at :263 that did not go on to :268) and the HLLE fallback by p_inter < 0 (the calls at :282 less those) in
each step, all sweep directions together, read with gcov from runs of the --coverage build to nlim = 1, 2, 3 (differences of the
cumulative counts) -- after asserting that build's final state equal to the normal build's bit for bit.

Fixtures are DATA; no reference text is stored.
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import REF, REFBIN, ROOT, read_rst, read_rst_levels      # noqa: E402
import hydromatrix as hm      # noqa: E402

BLAST3D = os.path.join(REF, "tst/3D-hydro/athinput.blast")
BLAST2D = os.path.join(REF, "tst/2D-hydro/athinput.blast")
RST_ONLY = ["job/maxout=1", "output1/out_fmt=rst", "output1/dt=1e300"]
ROE_LINES = (216, 227, 263, 268, 282)
COV = os.path.join(REFBIN, "cov")


# the NSCALARS = 1 configuration (oracle/Makefile.ref HMCFG_SCAL) of every scalar-free one the scalar fixtures are made from
SCAL_REF = {"blast": "sphere_hydro", "blast_noh": "sphere_hydro_noh", "blast_vl": "sphere_hydro_vl", "blast_ppm": "sphere_hydro_ppm",
            "blast_vl_ppm": "sphere_hydro_vl_ppm", "blast_smr": "sphere_hydro_smr"}


def build(targets=("hydromatrix", "hydromatrix_cov")):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-f", "Makefile.ref"] + list(targets), stdout=subprocess.DEVNULL)


def deck_with_keys(deck0, dvac, pvac, seed=0):
    """the reference's deck with the keys of our problem file added to its <problem> block"""
    tmp = tempfile.mkdtemp(prefix="golden_deck_")
    deck = os.path.join(tmp, "athinput.hydromatrix")
    text, n = re.subn(r"(?m)^(radius\s*=.*)$", r"\1\ndvac = %r\npvac = %r\nseed = %d" % (dvac, pvac, seed), open(deck0).read(), count=1)
    assert n == 1
    open(deck, "w").write(text)
    return tmp, deck


def run(exe, deck, args):
    tmp = tempfile.mkdtemp(prefix="golden_hm_")
    rundir = os.path.join(tmp, "run")
    pr = subprocess.run([exe, "-i", deck, "-d", rundir] + RST_ONLY + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                        errors="replace", cwd=tmp)
    if pr.returncode != 0:
        raise RuntimeError(pr.stdout[-2000:] + pr.stderr[-2000:])
    rsts = sorted(os.path.join(rundir, f) for f in os.listdir(rundir) if f.endswith(".rst"))
    return tmp, rsts


def roe_counts(refcfg):
    """execution counts of ROE_LINES accumulated in the --coverage objects of configuration `refcfg`"""
    obj = os.path.join(COV, refcfg, "obj")
    out = subprocess.run(["gcov", "-t", "-o", os.path.join(obj, "s_roe.o"), os.path.join(REF, "src/rsolvers/roe.c")],
                         stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, cwd=obj, check=True).stdout
    counts = {}
    for line in out.splitlines():
        m = re.match(r"\s*([0-9#=\-\*]+)\*?:\s*(\d+):", line)
        if m and int(m.group(2)) in ROE_LINES:
            c = m.group(1).rstrip("*")
            counts[int(m.group(2))] = int(c) if c.isdigit() else 0
    assert sorted(counts) == sorted(ROE_LINES), counts
    by_density = counts[263] - counts[268]            # (the -O3 build keeps no count of its own for the two assignments of hlle_flag)
    return np.array([counts[216], counts[227], by_density, counts[282] - by_density], dtype=np.int64)


def coverage(refcfg, deck, args, read, final):
    """-> cov_roe [step][4]; asserts the --coverage build's state after NSTEP steps equal to `final` bit for bit"""
    obj = os.path.join(COV, refcfg, "obj")
    cum = []
    for nlim in range(1, hm.NSTEP + 1):
        for f in os.listdir(obj):
            if f.endswith(".gcda"):
                os.remove(os.path.join(obj, f))
        tmp, rsts = run(os.path.join(COV, "athena_hydromatrix_" + refcfg), deck, args + [f"time/nlim={nlim}"])
        try:
            if nlim == hm.NSTEP:
                assert final(read(rsts[-1])), (refcfg, "the --coverage build computes another state")
        finally:
            shutil.rmtree(tmp)
        cum.append(roe_counts(refcfg))
    return np.diff(np.array([np.zeros(4, dtype=np.int64)] + cum), axis=0)


def single_level(only=None):
    """writes the single-level fixtures; only = (cfg, nx): -> (name, the arrays) of that one, nothing written"""
    for cfg, (refcfg, integ, order, cour, dvac, pvac) in hm.CFG.items():
        shapes = [(nx, BLAST3D) for nx in hm.SHAPES_3D]
        if cfg in hm.CFG_2D:
            shapes += [((nx[0], nx[1], 1), BLAST2D) for nx in hm.SHAPES_2D]
        for nx, deck0 in shapes:
            if only and only != (cfg, tuple(nx)):
                continue
            dtmp, deck = deck_with_keys(deck0, dvac, pvac)
            phys = ["job/num_domains=1"] + hm.overrides(nx, cour)
            tmp, rsts = run(os.path.join(REFBIN, "athena_hydromatrix_" + refcfg), deck, phys + [f"time/nlim={hm.NSTEP}"])
            first, last = read_rst(rsts[0], nx, 0, False), read_rst(rsts[-1], nx, 0, False)
            shutil.rmtree(tmp)
            assert last["nstep"] == hm.NSTEP
            assert np.isfinite(last["U"]).all() and (last["U"][..., 0] > 0).all() and (first["U"][..., 0] > 0).all()
            cov = coverage(refcfg, deck, phys, lambda p: read_rst(p, nx, 0, False), lambda r: np.array_equal(r["U"], last["U"]) and r["dt"] == last["dt"])
            shutil.rmtree(dtmp)
            name = f"hydromatrix_{cfg}_" + "x".join(str(n) for n in (nx if nx[2] > 1 else nx[:2])) + f"_n{hm.NSTEP}"
            out = os.path.join(HERE, name + ".npz")
            d = dict(nx=np.array(nx), U0=first["U"][..., :5], U=last["U"][..., :5], nstep=last["nstep"], time=last["time"],
                     dt=last["dt"], dt0=first["dt"], niter=np.array([], dtype=np.int64), overrides=np.array(hm.overrides(nx, cour)[3:]),
                     cfg=cfg, dvac=dvac, pvac=pvac, cov_roe=cov)
            if only:
                return name, d
            np.savez_compressed(out, **d)
            print(f"{name}: time={last['time']:.17g} dt={last['dt']:.17g} {os.path.getsize(out)} bytes; roe.c counts per step {cov.tolist()}")


def refined():
    for tag, (refcfg, integ, case, cour, dvac, pvac) in hm.SMR_CFG.items():
        root, kids = case
        grids = [(0, root, (0, 0, 0))] + list(kids)
        nxs = [g[1] for g in grids]
        dtmp, deck = deck_with_keys(BLAST2D if root[2] == 1 else BLAST3D, dvac, pvac)
        phys = hm.smr_overrides(case, cour)
        tmp, rsts = run(os.path.join(REFBIN, "athena_hydromatrix_" + refcfg), deck, phys + [f"time/nlim={hm.NSTEP}"])
        first, last = read_rst_levels(rsts[0], nxs, 0, False), read_rst_levels(rsts[-1], nxs, 0, False)
        shutil.rmtree(tmp)
        assert last["nstep"] == hm.NSTEP

        def same(r):
            return r["dt"] == last["dt"] and all(np.array_equal(a[0], b[0]) for a, b in zip(r["levels"], last["levels"]))
        cov = coverage(refcfg, deck, phys, lambda p: read_rst_levels(p, nxs, 0, False), same)
        shutil.rmtree(dtmp)
        # the reference's own 1-ulp twins of this run: how far they part from it, and in how many zones beyond 1e-9
        twin_spread, twin_nflip = 0.0, 0
        for seed in hm.REF_TWIN_SEEDS:
            dtmp, tdeck = deck_with_keys(BLAST2D if root[2] == 1 else BLAST3D, dvac, pvac, seed)
            tmp, rsts = run(os.path.join(REFBIN, "athena_hydromatrix_" + refcfg), tdeck, phys + [f"time/nlim={hm.NSTEP}"])
            twin = read_rst_levels(rsts[-1], nxs, 0, False)
            shutil.rmtree(tmp); shutil.rmtree(dtmp)
            errs = [np.abs(a[0][..., :5] - b[0][..., :5]) / np.abs(b[0][..., :5]).max(axis=(0, 1, 2)) for a, b in zip(twin["levels"], last["levels"])]
            assert all(np.isfinite(e).all() for e in errs), (tag, seed)
            twin_spread = max(twin_spread, max(float(e.max()) for e in errs))
            twin_nflip = max(twin_nflip, sum(int((e > 1e-9).any(axis=-1).sum()) for e in errs))
        d = dict(nlevels=len(grids), nxs=np.array(nxs), levels=np.array([g[0] for g in grids]), disp=np.array([g[2] for g in grids]),
                 nstep=last["nstep"], time=last["time"], dt=last["dt"], dt0=first["dt"], integrator=integ, overrides=np.array(phys),
                 tag=tag, dvac=dvac, pvac=pvac, cov_roe=cov, ref_twin_spread=twin_spread, ref_twin_nflip=twin_nflip)
        for l, ((U0, _), (U, _)) in enumerate(zip(first["levels"], last["levels"])):
            assert np.isfinite(U).all() and (U[..., 0] > 0).all() and (U0[..., 0] > 0).all(), (tag, l)
            d[f"U0_{l}"], d[f"U_{l}"] = U0[..., :5], U[..., :5]
        out = os.path.join(HERE, f"hydromatrix_smr_{tag}_n{hm.NSTEP}.npz")
        np.savez_compressed(out, **d)
        print(f"hydromatrix_smr_{tag}: time={last['time']:.17g} dt={last['dt']:.17g} {os.path.getsize(out)} bytes; roe.c counts per step {cov.tolist()}; "
              f"the reference's 1-ulp twins part by {twin_spread:.3e}, {twin_nflip} zones beyond 1e-9")


def check_unchanged(cfg="ctu", nx=(67, 10, 9)):
    """the problem file as it stands, compiled without a scalar, gives the committed fixture: every array, byte for byte"""
    name, d = single_level(only=(cfg, nx))
    old = np.load(os.path.join(HERE, name + ".npz"))
    assert sorted(old.files) == sorted(d), (sorted(old.files), sorted(d))
    for k in old.files:
        new = np.asarray(d[k])
        assert new.dtype == old[k].dtype and new.shape == old[k].shape and new.tobytes() == old[k].tobytes(), (name, k)
    print(f"{name}: regenerated, all {len(old.files)} arrays byte for byte the committed ones")


def concentration(U):
    return U[..., 5] / U[..., 0]


def scalar_single():
    for cfg in hm.SCAL_CFG:
        refcfg0, integ, order, cour, dvac, pvac = hm.CFG[cfg]
        refcfg = SCAL_REF[refcfg0]
        for nx in hm.SHAPES_3D:
            base_name = hm.fixture_name(cfg, nx)
            base = np.load(os.path.join(HERE, base_name + ".npz"))
            dtmp, deck = deck_with_keys(BLAST3D, dvac, pvac)
            phys = ["job/num_domains=1"] + hm.overrides(nx, cour)
            tmp, rsts = run(os.path.join(REFBIN, "athena_hydromatrix_" + refcfg), deck, phys + [f"time/nlim={hm.NSTEP}"])
            first, last = read_rst(rsts[0], nx, 1, False), read_rst(rsts[-1], nx, 1, False)
            shutil.rmtree(tmp)
            assert last["nstep"] == hm.NSTEP
            assert np.isfinite(last["U"]).all() and (last["U"][..., 0] > 0).all()
            assert np.array_equal(first["U"], hm.pattern(nx, hm.gamma(nx[2]), dvac=dvac, pvac=pvac, nscal=1)), "the numpy twin of the problem file"
            cov = coverage(refcfg, deck, phys, lambda p: read_rst(p, nx, 1, False), lambda r: np.array_equal(r["U"], last["U"]) and r["dt"] == last["dt"])
            shutil.rmtree(dtmp)
            passive = (np.array_equal(first["U"][..., :5], base["U0"]) and np.array_equal(last["U"][..., :5], base["U"])
                       and first["dt"] == float(base["dt0"]) and last["dt"] == float(base["dt"]) and last["time"] == float(base["time"])
                       and np.array_equal(cov, base["cov_roe"]))
            r = concentration(last["U"])
            name = hm.fixture_name(cfg, nx, 1)
            out = os.path.join(HERE, name + ".npz")
            if passive:
                np.savez_compressed(out, s0=first["U"][..., 5], s=last["U"][..., 5], base=base_name, nscal=1, conc_range=np.array([r.min(), r.max()]))
            else:
                np.savez_compressed(out, nx=np.array(nx), U0=first["U"], U=last["U"], nstep=last["nstep"], time=last["time"], dt=last["dt"],
                                    dt0=first["dt"], niter=np.array([], dtype=np.int64), overrides=np.array(hm.overrides(nx, cour)[3:]), cfg=cfg,
                                    dvac=dvac, pvac=pvac, cov_roe=cov, nscal=1, conc_range=np.array([r.min(), r.max()]))
            print(f"{name} ({refcfg}): hydro columns, dt0, dt, time, roe.c counts equal to {base_name} bit for bit: {passive}; "
                  f"concentration {r.min():.6g} ... {r.max():.6g}; {os.path.getsize(out)} bytes")


def scalar_refined():
    for tag in hm.SCAL_SMR:
        refcfg0, integ, case, cour, dvac, pvac = hm.SMR_CFG[tag]
        refcfg = SCAL_REF[refcfg0]
        root, kids = case
        grids = [(0, root, (0, 0, 0))] + list(kids)
        nxs = [g[1] for g in grids]
        base_name = hm.smr_fixture_name(tag)
        base = np.load(os.path.join(HERE, base_name + ".npz"))
        exe = os.path.join(REFBIN, "athena_hydromatrix_" + refcfg)
        dtmp, deck = deck_with_keys(BLAST3D, dvac, pvac)
        phys = hm.smr_overrides(case, cour)
        tmp, rsts = run(exe, deck, phys + [f"time/nlim={hm.NSTEP}"])
        first, last = read_rst_levels(rsts[0], nxs, 1, False), read_rst_levels(rsts[-1], nxs, 1, False)
        shutil.rmtree(tmp)
        assert last["nstep"] == hm.NSTEP

        def same(r):
            return r["dt"] == last["dt"] and all(np.array_equal(a[0], b[0]) for a, b in zip(r["levels"], last["levels"]))
        cov = coverage(refcfg, deck, phys, lambda p: read_rst_levels(p, nxs, 1, False), same)
        shutil.rmtree(dtmp)
        passive = (first["dt"] == float(base["dt0"]) and last["dt"] == float(base["dt"]) and last["time"] == float(base["time"])
                   and np.array_equal(cov, base["cov_roe"])
                   and all(np.array_equal(U0[..., :5], base[f"U0_{l}"]) and np.array_equal(U[..., :5], base[f"U_{l}"])
                           for l, ((U0, _), (U, _)) in enumerate(zip(first["levels"], last["levels"]))))
        assert passive, (tag, "the scalar run's hydro columns part from the scalar-free fixture's: store it whole")
        # the reference's own 1-ulp twins of the six-variable run, over six columns
        twin_spread, twin_nflip = 0.0, 0
        for seed in hm.REF_TWIN_SEEDS:
            dtmp, tdeck = deck_with_keys(BLAST3D, dvac, pvac, seed)
            tmp, rsts = run(exe, tdeck, phys + [f"time/nlim={hm.NSTEP}"])
            twin = read_rst_levels(rsts[-1], nxs, 1, False)
            shutil.rmtree(tmp); shutil.rmtree(dtmp)
            errs = [np.abs(a[0] - b[0]) / np.abs(b[0]).max(axis=(0, 1, 2)) for a, b in zip(twin["levels"], last["levels"])]
            assert all(np.isfinite(e).all() for e in errs), (tag, seed)
            twin_spread = max(twin_spread, max(float(e.max()) for e in errs))
            twin_nflip = max(twin_nflip, sum(int((e > 1e-9).any(axis=-1).sum()) for e in errs))
        rs = [concentration(U) for U, _ in last["levels"]]
        d = dict(base=base_name, nscal=1, conc_range=np.array([min(r.min() for r in rs), max(r.max() for r in rs)]),
                 ref_twin_spread=twin_spread, ref_twin_nflip=twin_nflip)
        for l, ((U0, _), (U, _)) in enumerate(zip(first["levels"], last["levels"])):
            g = grids[l]
            assert np.isfinite(U).all() and (U[..., 0] > 0).all(), (tag, l)
            assert np.array_equal(U0, hm.pattern(g[1], hm.gamma(root[2]), g[0], g[2], dvac, pvac, 1)), "the numpy twin of the problem file"
            d[f"s0_{l}"], d[f"s_{l}"] = U0[..., 5], U[..., 5]
        name = hm.smr_fixture_name(tag, 1)
        out = os.path.join(HERE, name + ".npz")
        np.savez_compressed(out, **d)
        print(f"{name} ({refcfg}): hydro columns, dt0, dt, time, roe.c counts equal to {base_name} bit for bit: {passive}; concentration "
              f"{d['conc_range'][0]:.6g} ... {d['conc_range'][1]:.6g}; the reference's 1-ulp twins of the six-variable run part by "
              f"{twin_spread:.3e}, {twin_nflip} zones beyond 1e-9; {os.path.getsize(out)} bytes")


def main():
    """arguments: any of single, smr (the scalar-free fixtures), scalar (the hydromatrix_s1_* ones, from the committed scalar-free
    ones), check (one scalar-free fixture regenerated and compared); nobuild.  Default: single smr scalar"""
    if not os.path.isdir(REF):
        sys.exit("needs the reference tree")
    what = [a for a in sys.argv[1:] if a != "nobuild"] or ["single", "smr", "scalar"]
    if "nobuild" not in sys.argv[1:]:
        build(("hydromatrix", "hydromatrix_cov") + (("hydromatrix_scal", "hydromatrix_scal_cov") if "scalar" in what else ()))
    if "single" in what:
        single_level()
    if "smr" in what:
        refined()
    if "check" in what:
        check_unchanged()
    if "scalar" in what:
        scalar_single()
        scalar_refined()


if __name__ == "__main__":
    main()
