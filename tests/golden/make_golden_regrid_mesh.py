"""Regenerates tests/golden/regridmesh_*.npz: restart dumps of the UNMODIFIED reference built with --enable-mpi --enable-smr
(oracle/Makefile.ref: athena_blast_smr_mpi, athena_ioniz_sphere_smr_mpi) on decompositions that cut every <domainN> differently
-- x1 cuts, uneven Grids and ranks without a Grid of the root among them -- and what the reference made of them when it was
continued with ``-r`` on the same cuts.  TEST INFRASTRUCTURE: needs the reference tree and oracle/_ref; the tests only read the
.npz files.  It runs only executables under oracle/_ref and stores only what they wrote.

The rules by which the files of a run are joined are written out here once more, independently of the package
(restart.mesh_grid_boxes is what the tests check against these files):
  A  every Domain -- level by level, deck order inside a level -- is cut by its own NGrid_x1/2/3 into Grids of Nx / NGrid zones,
     the whole remainder of a direction on the first Grid of that direction (init_mesh.c:505-662);
  B  the Grids take consecutive world ranks, x1 index fastest, then x2, then x3; the count runs on from Domain to Domain and wraps
     at the number of processes (:589-590), it ends at 0 (:661), and no Domain has more Grids than there are ranks (:564-567);
  C  rank r writes id<r>/<base>[-id<r>].NNNN.rst with the sections of the Grids it holds in that same order (restart.c:531-770).
EdgeFlux: two Grids hold an entry for the face they share; the join takes the upper Grid's, and the last face of a direction from
the last Grid of the Domain.

A fixture holds
  problem, nranks, overrides, blocks      the run (overrides as given to the reference on its command line)
  domains [nd][7]                         level, Nx1..3, iDisp, jDisp, kDisp of every Domain in the order of rule A
  ngrid [nd][3]                           its NGrid_x1..3
  seed_names, seed_<i>                    the restart dumps of one number of all ranks (relative paths, rank order; raw bytes)
  seed_nstep, seed_time, seed_dt          rank 0's
and, where the run was continued (``-r`` on the seeds, same ranks and cuts):
  final_U<n>, final_EF<n>                 the last restart dump of the continued run, joined per Domain by rules A to C
  final_time, final_dt, final_nstep, nlim
  niter [steps][levels]                   radiation sub-cycles of every step of the continued run, as rank 0 printed them
  D_ref [nd][6]                           (sphere2_x2x3) per Domain and field: max |final - final of the 1x1x2 run| / field maximum

The generator asserts what is true of the reference alone and fails if it is not: every zone of every Domain is covered once by
the Grids of rules A and B; no NaN in any payload; for the blast cases the same deck on 1 x 1 x 2 in every Domain gives the same
joined seeds and the same joined final state, bit for bit with time and dt; for sphere2_x2x3 D_ref <= 1e-10 in d, E, s and <= 1e-5
in the momenta and identical sub-cycle counts; both levels sub-cycle more than once in every stored sphere step.  `findings` as
first argument also runs the decompositions that no fixture keeps and prints all four findings of DESIGN.md section 7."""
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, REFBIN, read_rst_levels               # noqa: E402
from make_golden_dumps import BLAST, MPIEXEC, SPHERE                # noqa: E402
from make_golden_meshdriver import SPHERE_L1, SPHERE_NX, SPHERE_OVER      # noqa: E402

FIELDS = ("d", "M1", "M2", "M3", "E", "s")


# ---- rules A to C ------------------------------------------------------------------------------------------------------------
def cut(Nx, ngrid):
    """rule A: [(disp, nx)] relative to the Domain, x1 index fastest"""
    sz, dp = [], []
    for d in range(3):
        q, r = divmod(Nx[d], ngrid[d])
        s = [q + r] + [q] * (ngrid[d] - 1)
        sz.append(s); dp.append([sum(s[:i]) for i in range(ngrid[d])])
    return [((dp[0][l], dp[1][m], dp[2][n]), (sz[0][l], sz[1][m], sz[2][n]))
            for n in range(ngrid[2]) for m in range(ngrid[1]) for l in range(ngrid[0])]


def deal(domains, ngrids, nproc):
    """rule B: per Domain [(rank, disp, nx)]"""
    out, nxt = [], 0
    for dom, ng in zip(domains, ngrids):
        boxes = cut(dom[1:4], ng)
        assert len(boxes) <= nproc
        row = []
        for disp, nx in boxes:
            row.append((nxt, disp, nx)); nxt = (nxt + 1) % nproc
        out.append(row)
    assert nxt == 0
    return out


def rank_of(rel):
    m = re.search(r"-id(\d+)\.", os.path.basename(rel))
    return int(m.group(1)) if m else 0


def files_of(rundir, num):
    """rule C: the restart dumps of number `num` in rank order (relative paths)"""
    rel = sorted((p for p in tree(rundir) if p.endswith(".%04d.rst" % num)), key=rank_of)
    assert [rank_of(p) for p in rel] == list(range(len(rel))) and all(p.startswith("id%d/" % r) for r, p in enumerate(rel)), rel
    return rel


def join(rundir, rels, domains, ngrids, nscal, ion):
    """-> ([(U, EdgeFlux or None)] per Domain, time, dt, nstep); every zone covered once, every face at least once"""
    nproc = len(rels)
    table = deal(domains, ngrids, nproc)
    per_rank = []
    for r, rel in enumerate(rels):
        mine = [(n, b) for n, row in enumerate(table) for b in row if b[0] == r]
        g = read_rst_levels(os.path.join(rundir, rel), [b[2] for _n, b in mine], nscal, ion)
        assert os.path.getsize(os.path.join(rundir, rel)) == expected_size(os.path.join(rundir, rel), [b[2] for _n, b in mine], nscal, ion), rel
        per_rank.append((g, {n: st for (n, _b), st in zip(mine, g["levels"])}))
    t0 = per_rank[0][0]
    assert all((g["time"], g["dt"], g["nstep"]) == (t0["time"], t0["dt"], t0["nstep"]) for g, _ in per_rank)
    out = []
    for n, (dom, row) in enumerate(zip(domains, table)):
        Nx = dom[1:4]
        U = np.zeros((Nx[2], Nx[1], Nx[0], 6)); cover = np.zeros((Nx[2], Nx[1], Nx[0]), dtype=int)
        ef = np.zeros((Nx[2] + 1, Nx[1] + 1, Nx[0] + 1)) if ion else None
        fcover = np.zeros(ef.shape, dtype=int) if ion else None
        for rank, lo, nx in sorted(row, key=lambda b: (b[1][2], b[1][1], b[1][0])):          # lower Grids first
            Ug, eg = per_rank[rank][1][n]
            assert not np.isnan(Ug).any() and (eg is None or not np.isnan(eg).any()), (n, rank)
            sl = tuple(slice(lo[d], lo[d] + nx[d]) for d in (2, 1, 0))
            U[sl] = Ug; cover[sl] += 1
            if ion:
                sl = tuple(slice(lo[d], lo[d] + nx[d] + 1) for d in (2, 1, 0))
                ef[sl] = eg; fcover[sl] = 1
        assert np.all(cover == 1) and (not ion or np.all(fcover == 1)), n
        out.append((U[..., :5 + nscal], ef))
    return out, t0["time"], t0["dt"], t0["nstep"]


def expected_size(path, nxs, nscal, ion):
    b = open(path, "rb").read()
    pos = b.index(b"\nTIME_STEP\n") + 11 + 8
    for nx in nxs:
        n = nx[0] * nx[1] * nx[2]
        for lab in ("DENSITY", "1-MOMENTUM", "2-MOMENTUM", "3-MOMENTUM", "ENERGY"):
            pos += len(lab) + 2 + 8 * n
        if ion:
            pos += len("EDGEFLUX") + 2 + 8 * (nx[0] + 1) * (nx[1] + 1) * (nx[2] + 1)
        for s in range(nscal):
            pos += len("SCALAR %d" % s) + 2 + 8 * n
    return pos + len("\nUSER_DATA\n")


# ---- running the reference ---------------------------------------------------------------------------------------------------
def tree(rundir):
    return sorted(os.path.relpath(os.path.join(dp, f), rundir) for dp, _, fs in os.walk(rundir) for f in fs)


def deck_copy(deck, path, ngrids, blocks):
    """the reference's deck with NGrid_x* of every <domainN> and `blocks` as its only <outputN> blocks (neither can be given on the
    command line: par_cmdline refuses a block or key the deck does not hold)"""
    txt = open(deck).read()
    txt = re.sub(r"(?m)^\s*(NGrid_x[123]|AutoWithNProc)\s*=.*\n", "", txt)
    txt = re.sub(r"(?ms)^<output\d+>.*?(?=^<)", "", txt)
    for n, ng in enumerate(ngrids, 1):
        assert f"<domain{n}>" in txt
        txt = txt.replace(f"<domain{n}>", f"<domain{n}>\nNGrid_x1 = {ng[0]}\nNGrid_x2 = {ng[1]}\nNGrid_x3 = {ng[2]}", 1)
    txt = re.sub(r"(?m)^maxout\s*=.*$", "maxout = %d" % max(int(k) for k in blocks), txt, count=1)
    for n, kv in sorted(blocks.items(), key=lambda t: int(t[0])):
        txt += f"\n<output{n}>\n" + "".join(f"{k} = {v}\n" for k, v in kv.items())
    open(path, "w").write(txt)


def execute(exe, args, nranks, cwd):
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/conda/lib:" + env.get("LD_LIBRARY_PATH", "")
    cmd = [MPIEXEC, "-prepend-rank", "-n", str(nranks), os.path.join(REFBIN, exe)] + args
    pr = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=cwd, env=env, timeout=1800)
    if pr.returncode != 0:
        raise RuntimeError(pr.stdout[-2000:] + pr.stderr[-2000:])
    assert "Neg or NaN" not in pr.stdout + pr.stderr
    return pr


def sub_cycles(pr, nlev):
    n = [int(m) for m in re.findall(r"(?m)^\[0\].*Radiation done in (\d+) iterations", pr.stdout + pr.stderr)]
    assert len(n) % nlev == 0, len(n)
    return np.array(n, dtype=np.int64).reshape(-1, nlev)


def dump_at_step(rundir, step):
    """the number of the LAST restart dump of rank 0 that holds step `step`"""
    best = None
    for rel in tree(rundir):
        if rel.startswith("id0/") and rel.endswith(".rst"):
            b = open(os.path.join(rundir, rel), "rb").read(1 << 16)
            pos = b.index(b"N_STEP\n") + 7
            if int(np.frombuffer(b, "<i4", 1, pos)[0]) == step:
                best = int(rel.rsplit(".", 2)[1])
    assert best is not None, (step, tree(rundir))
    return best


class Deck:
    """one problem on one mesh: `over` gives the Domains (job/num_domains, domainN/...), `blocks` the one restart block"""

    def __init__(self, exe, deck, problem, domains, over, blocks, nscal=0, ion=False):
        self.exe, self.deck, self.problem, self.domains, self.over, self.blocks = exe, deck, problem, domains, list(over), blocks
        self.nscal, self.ion = nscal, ion
        self.nlev = 1 + max(d[0] for d in domains)

    def run(self, tmp, tag, ngrids, nranks, nlim, seed_step, cont=True):
        """the run to `seed_step` + the dump of that step; with cont the run continued from it to `nlim` by ``-r`` on the same
        ranks.  -> dict(rundir, seed_rel, seeds (joined), head (time, dt, nstep), final (joined), ftime (time, dt, nstep), niter)"""
        full, res, seeds = (os.path.join(tmp, tag + x) for x in ("_full", "_resumed", "_seeds"))
        deck_used = os.path.join(tmp, tag + "_athinput")
        deck_copy(self.deck, deck_used, ngrids, self.blocks)
        execute(self.exe, ["-i", deck_used, "-d", full, f"time/nlim={seed_step}"] + self.over, nranks, tmp)
        num = dump_at_step(full, seed_step)
        rel = files_of(full, num)
        assert len(rel) == nranks, rel
        S, t, dt, ns = join(full, rel, self.domains, ngrids, self.nscal, self.ion)
        assert ns == seed_step
        out = dict(rundir=full, seed_rel=rel, seeds=S, head=(t, dt, ns))
        if not cont:
            return out
        os.makedirs(seeds)
        for p in rel:
            shutil.copy(os.path.join(full, p), os.path.join(seeds, os.path.basename(p)))
        pr = execute(self.exe, ["-r", os.path.join(seeds, os.path.basename(rel[0])), "-d", res, f"time/nlim={nlim}"], nranks, tmp)
        last = dump_at_step(res, nlim)
        F, t, dt, ns = join(res, files_of(res, last), self.domains, ngrids, self.nscal, self.ion)
        assert ns == nlim
        out.update(final=F, ftime=(t, dt, ns), niter=sub_cycles(pr, self.nlev) if self.ion else np.zeros((0, self.nlev), dtype=np.int64))
        if self.ion:
            assert len(out["niter"]) == nlim - seed_step and out["niter"].min() > 1, out["niter"]
        return out


def bits_equal(A, B):
    """joined states [(U, ef)]: every double the same"""
    return all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) and
               (ea is None or np.array_equal(ea.view(np.uint64), eb.view(np.uint64))) for (a, ea), (b, eb) in zip(A, B))


def spread(A, B):
    """[nd][nvar]: max |A - B| / max |B| per Domain and field"""
    out = []
    for (a, _), (b, _) in zip(A, B):
        scale = np.abs(b).max(axis=(0, 1, 2)); scale[scale == 0] = 1.0
        out.append(np.abs(a - b).max(axis=(0, 1, 2)) / scale)
    return np.array(out)


def ef_diff(A, B):
    """(entries that differ, largest difference / the largest entry of that Domain) of EdgeFlux over all Domains"""
    n, m = 0, 0.0
    for (_, a), (_, b) in zip(A, B):
        n += int(np.count_nonzero(a != b)); m = max(m, float(np.abs(a - b).max() / np.abs(b).max()))
    return n, m


def store(name, deck, ngrids, nranks, r, nlim=None, extra=None):
    d = dict(problem=deck.problem, nranks=nranks, overrides=np.array(deck.over), blocks=json.dumps(deck.blocks),
             domains=np.array(deck.domains, dtype=np.int64), ngrid=np.array(ngrids, dtype=np.int64),
             seed_names=np.array(r["seed_rel"]), seed_time=r["head"][0], seed_dt=r["head"][1], seed_nstep=r["head"][2])
    for i, p in enumerate(r["seed_rel"]):
        d[f"seed_{i}"] = np.frombuffer(open(os.path.join(r["rundir"], p), "rb").read(), dtype=np.uint8)
    if "final" in r:
        for n, (U, ef) in enumerate(r["final"]):
            d[f"final_U{n}"] = U
            if ef is not None:
                d[f"final_EF{n}"] = ef
        d["final_time"], d["final_dt"], d["final_nstep"] = r["ftime"]
        d["nlim"] = nlim
        d["niter"] = r["niter"]
    d.update(extra or {})
    out = os.path.join(HERE, name + ".npz")
    np.savez_compressed(out, **d)
    print(f"{name}: {nranks} ranks, NGrid {[tuple(g) for g in ngrids]}, seeds at step {r['head'][2]}"
          + (f", continued to {r['ftime'][2]}" if "final" in r else "") + f"; {os.path.getsize(out)} bytes")


def dom(n, nx, disp=None, level=None):
    o = [f"domain{n}/Nx{d + 1}={nx[d]}" for d in range(3)]
    if disp:
        o += [f"domain{n}/{k}Disp={disp[d]}" for d, k in enumerate("ijk")]
    if level is not None:
        o += [f"domain{n}/level={level}"]
    return o


RST_EVERY_PASS = {"1": {"out_fmt": "rst", "dt": "1e-6"}}      # an interval far below a step: every pass of the loop writes

BLAST2 = Deck("athena_blast_smr_mpi", BLAST, "blast", [(0, 16, 12, 16, 0, 0, 0), (1, 16, 12, 16, 8, 6, 8)],
              ["job/num_domains=2"] + dom(1, (16, 12, 16)) + dom(2, (16, 12, 16), (8, 6, 8)), RST_EVERY_PASS)
BLAST3 = Deck("athena_blast_smr_mpi", BLAST, "blast", [(0, 22, 12, 18, 0, 0, 0), (1, 20, 12, 16, 10, 6, 12), (2, 16, 8, 12, 32, 20, 36)],
              ["job/num_domains=3"] + dom(1, (22, 12, 18)) + dom(2, (20, 12, 16), (10, 6, 12)) + dom(3, (16, 8, 12), (32, 20, 36)),
              RST_EVERY_PASS)
SPHERE2 = Deck("athena_ioniz_sphere_smr_mpi", SPHERE, "ioniz_sphere", [(0,) + SPHERE_NX + (0, 0, 0), (1,) + SPHERE_L1],
               ["job/num_domains=2"] + dom(1, SPHERE_NX) + dom(2, SPHERE_L1[:3], SPHERE_L1[3:]) + SPHERE_OVER, RST_EVERY_PASS,
               nscal=1, ion=True)
# the Domains of smr_blast_2dom_s6 (make_golden.py): two level-1 patches
BLAST2DOM = Deck("athena_blast_smr_mpi", BLAST, "blast",
                 [(0, 16, 24, 16, 0, 0, 0), (1, 12, 16, 20, 8, 20, 6), (1, 6, 8, 8, 22, 24, 10)],
                 ["job/num_domains=3"] + dom(1, (16, 24, 16)) + dom(2, (12, 16, 20), (8, 20, 6)) + dom(3, (6, 8, 8), (22, 24, 10), level=1),
                 RST_EVERY_PASS)
Z = (1, 1, 2)


def main():
    if not os.path.isdir(REF) or not os.path.isdir(REFBIN):
        sys.exit("needs the reference tree and oracle/_ref (make -C oracle -f Makefile.ref blast_smr_mpi ioniz_sphere_smr_mpi)")
    args = sys.argv[1:]
    findings = bool(args) and args[0] == "findings"
    only = args[1:] if findings else args
    want = lambda name: not only or name in only      # noqa: E731
    tmp = tempfile.mkdtemp(prefix="golden_regridmesh_")
    try:
        # ---- finding 1: blast, two levels ----
        base2 = None
        if want("blast2_x1x3") or want("blast2_noroot") or findings:
            base2 = BLAST2.run(tmp, "b2z", [Z, Z], 2, 7, 3)
        for name, ngrids, nranks in (("blast2_x1x3", [(2, 1, 2), (1, 2, 2)], 4), ("blast2_noroot", [Z, Z], 4)):
            if want(name):
                r = BLAST2.run(tmp, name, ngrids, nranks, 7, 3)
                assert bits_equal(r["seeds"], base2["seeds"]) and r["head"] == base2["head"], name
                assert bits_equal(r["final"], base2["final"]) and r["ftime"] == base2["ftime"], name
                store("regridmesh_" + name, BLAST2, ngrids, nranks, r, 7)
        if findings:
            same = []
            z0 = BLAST2.run(tmp, "b2z0", [Z, Z], 2, 7, 0, cont=False)
            others = (([(2, 1, 2), (1, 2, 2)], 4), ([Z, Z], 4), ([(1, 2, 2), (2, 2, 1)], 4), ([(2, 1, 1), Z], 2), ([(2, 2, 1), (2, 1, 2)], 4),
                      ([(2, 2, 2), (2, 2, 2)], 8))
            for ngrids, nranks in others:
                r0 = BLAST2.run(tmp, "b2f%d" % len(same), ngrids, nranks, 7, 0, cont=False)
                r = BLAST2.run(tmp, "b2g%d" % len(same), ngrids, nranks, 7, 3)
                same.append(bits_equal(r0["seeds"], z0["seeds"]) and r0["head"] == z0["head"] and
                            bits_equal(r["final"], base2["final"]) and r["ftime"] == base2["ftime"])
            print(f"finding 1 (blast, two levels): against 2 ranks 1x1x2 / 1x1x2, U of both levels, time and dt at step 0 and at step 7 "
                  f"(continued from step 3) bit for bit equal on 2x1x2/1x2x2 (4 ranks), 1x1x2/1x1x2 (4 ranks: 2 and 3 without a root "
                  f"Grid), 1x2x2/2x2x1 (4), 2x1x1/1x1x2 (2), 2x2x1/2x1x2 (4), 2x2x2/2x2x2 (8): {same}")
            assert all(same)
        # ---- finding 2: blast, three levels ----
        if want("blast3_uneven"):
            ngrids = [(4, 1, 1), (1, 2, 2), (2, 1, 2)]
            base3 = BLAST3.run(tmp, "b3z", [Z, Z, Z], 2, 6, 2)
            r = BLAST3.run(tmp, "b3", ngrids, 4, 6, 2)
            assert [b[1][0] for b in cut((22, 12, 18), (4, 1, 1))] == [7, 5, 5, 5]
            assert bits_equal(r["seeds"], base3["seeds"]) and r["head"] == base3["head"]
            assert bits_equal(r["final"], base3["final"]) and r["ftime"] == base3["ftime"]
            store("regridmesh_blast3_uneven", BLAST3, ngrids, 4, r, 6)
            print("finding 2 (blast, three levels): 4 ranks 4x1x1 / 1x2x2 / 2x1x2 (x1 Grids of 7, 5, 5, 5 zones) against 2 ranks 1x1x2 on "
                  "every level: seeds at step 2 and the state at step 6 bit for bit equal, time and dt included")
        # ---- finding 3: the sphere ----
        bases = None
        if want("sphere2_x2x3") or (findings and want("sphere2_x1")):
            bases = SPHERE2.run(tmp, "sz", [Z, Z], 2, 4, 2)
        if want("sphere2_x2x3"):
            ngrids = [(1, 2, 2), (1, 2, 2)]
            r = SPHERE2.run(tmp, "s22", ngrids, 4, 4, 2)
            D = spread(r["final"], bases["final"])
            ne, me = ef_diff(r["final"], bases["final"])
            print(f"finding 3 (ioniz_sphere): 4 ranks 1x2x2 / 1x2x2 against 2 ranks 1x1x2 / 1x1x2 at step 4: D_ref per Domain "
                  f"{dict(zip(FIELDS, D.max(axis=0)))}; EdgeFlux differs in {ne} entries by at most {me:.3g} of the largest entry; sub-cycles {r['niter'].tolist()} "
                  f"against {bases['niter'].tolist()}")
            assert D[:, [0, 4, 5]].max() <= 1e-10 and D[:, 1:4].max() <= 1e-5, D
            assert np.array_equal(r["niter"], bases["niter"])
            store("regridmesh_sphere2_x2x3", SPHERE2, ngrids, 4, r, 4, dict(D_ref=D))
        if want("sphere2_x1"):
            ngrids = [(2, 1, 2), (2, 2, 1)]
            r = SPHERE2.run(tmp, "sx1", ngrids, 4, 4, 2, cont=findings)
            if findings:
                D = spread(r["final"], bases["final"])
                ne, me = ef_diff(r["final"], bases["final"])
                print(f"finding 3, x1 cuts: 4 ranks 2x1x2 / 2x2x1 against 2 ranks 1x1x2 / 1x1x2 at step 4: per field {dict(zip(FIELDS, D.max(axis=0)))}; "
                      f"EdgeFlux differs in {ne} entries by at most {me:.3g} of the largest entry; sub-cycles {r['niter'].tolist()} against {bases['niter'].tolist()}")
                for k in ("final", "ftime", "niter"):
                    r.pop(k)
            store("regridmesh_sphere2_x1", SPHERE2, ngrids, 4, r)
        # ---- finding 4: two Domains on one level ----
        if want("blast2dom"):
            ngrids = [(1, 2, 2), (1, 1, 2), (1, 2, 1)]
            r = BLAST2DOM.run(tmp, "b2d", ngrids, 4, 6, 2, cont=findings)
            if findings:
                z = np.load(os.path.join(HERE, "smr_blast_2dom_s6.npz"))
                serial = [(z[f"U{n}"][..., :5], None) for n in range(3)]
                two = BLAST2DOM.run(tmp, "b2d2", [Z, (1, 1, 1), (1, 1, 1)], 2, 6, 2)
                print(f"finding 4 (two Domains on level 1) at step 6 against the serial fixture smr_blast_2dom_s6: 2 ranks (root 1x1x2, each "
                      f"patch whole) {spread(two['final'], serial).max():.3g}; 4 ranks (root 1x2x2, patches 1x1x2 and 1x2x1) per Domain and field "
                      f"{spread(r['final'], serial).tolist()}")
                for k in ("final", "ftime", "niter"):
                    r.pop(k)
            store("regridmesh_blast2dom", BLAST2DOM, ngrids, 4, r)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
