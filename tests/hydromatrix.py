"""TEST INFRASTRUCTURE: the designed hydro state of tests/fixtures/hydro_matrix.c in numpy (the same expressions, operation by
operation), the oracle set up on it, and the names of the branch classes the oracle counts on it (oracle/athena_oracle.c,
orc_dbg_class).  Nothing under atmospheric-athena_amd/ may import this module.

The state is a function of the ROOT-zone indices (a, b, c) only -- a zone of a refined level carries its root zone's values, so
the four (eight) fine zones of a coarse one are exact copies and their restriction (a+a)+(a+a) times 0.25 is exact.  Blocks of BLK
root zones along each axis; the velocity along an axis is boosted block by block through the cycle SEQ = -1, +1, 0, +1 times VB
(about twice the sound speed), the cycles starting at different blocks along the three axes: blocks receding from each other at four and at two
sound speeds (where the Roe solver's intermediate states fail: the HLLE fallback), blocks running into gas at rest, supersonic
blocks of either sign along each axis (the upwind returns).  Every fifth block along the diagonal is a near-vacuum block -- the
receding flows run across it.  With PVAC < 0 its total energy lies below the kinetic energy (what an overshoot leaves behind):
the pressure floor of Cons1D_to_Prim1D then acts from the first step; only the configurations that survive it are run so.  A small
shear of all three velocities by integer patterns of co-prime periods keeps every momentum non-uniform and different per direction.

With a passive scalar (nscal = 1: the NS = 1 instantiations of every hydro kernel) the sixth column is s = d * r, the concentration
r = 0.125 + 0.125 * ((a + 3 b + 5 c) % 7): period 7, co-prime to the block cycle, another value across every face along each axis,
exact in binary.  The scalar is passive: the reference's hydro columns, dt and time of such a run equal the scalar-free run's bit for
bit (asserted by tests/golden/make_golden_hydromatrix.py), so a scalar fixture hydromatrix_s1_* stores the sixth column only and names
its base fixture; `load` puts the two together.

A failing GPU comparison is read with the census: the first differing zone's faces are classified by `face_classes` on the
state before the step (supersonic return, HLLE, Roe), which names the branch of the kernel to look at."""
import ctypes as C
import os

import numpy as np

import orc

BLK = 3
VB = (2.6, 2.4, 2.8)         # boost of a supersonic block along x1, x2, x3; the quiet gas has a sound speed of 1.0 ... 1.41
SEQ = (-1.0, 1.0, 0.0, 1.0)  # the boosts of four consecutive blocks along an axis, in units of VB (x1 starts one block on, x2 three)
DVAC, PVAC = 0.02, 0.004      # density and pressure of a near-vacuum block over the quiet gas'
PVAC_FLOOR = -1.0e-2         # the pressure factor of the runs that have to reach the pressure floor
NSTEP = 3

# the classes of orc_dbg_class, in its order (oracle/athena_oracle.c)
CLASSES = ("F=Fl", "F=Fr", "HLLE u0<=0", "HLLE p_inter<0", "etah wins a wave", "etah loses a wave", "limiter zero", "limiter 2 lim1",
           "limiter lim2", "clamp acts", "trace ev0>=0", "trace vx>=0", "trace vx<=0", "trace ev4<=0", "pressure floor",
           "ppm flat", "ppm steepened", "scalar from the left", "scalar from the right")
ROE = CLASSES[:4]
HCORR = CLASSES[4:6]
RECON = CLASSES[6:10]
TRACE = CLASSES[10:14]
PPM = CLASSES[15:17]
SCALAR = CLASSES[17:19]      # the Roe path's scalar flux: F[0] >= 0 takes the left state's concentration, F[0] < 0 the right's
MIN_COUNT = 32


def root_indices(nx, level=0, disp=(0, 0, 0)):
    """-> (a, b, c) root-zone indices of the active zones [k][j][i] of a Grid of nx zones at `level`, `disp` fine zones from the
    root's origin"""
    k, j, i = np.meshgrid(np.arange(nx[2]), np.arange(nx[1]), np.arange(nx[0]), indexing="ij")
    return (i + disp[0]) >> level, (j + disp[1]) >> level, (k + disp[2]) >> level


def boosts(a, b, c):
    """-> the block's boost along x1, x2, x3 in units of VB"""
    seq = np.array(SEQ)
    return seq[(a // BLK + 1) % 4], seq[(b // BLK + 3) % 4], seq[(c // BLK) % 4]


def near_vacuum(a, b, c):
    return (a // BLK + b // BLK + c // BLK) % 5 == 1


def concentration(a, b, c):
    """the scalar over the density of the root zone (a, b, c)"""
    return 0.125 + 0.125 * ((a + 3 * b + 5 * c) % 7).astype(np.float64)


def pattern(nx, gamma, level=0, disp=(0, 0, 0), dvac=DVAC, pvac=PVAC, nscal=0):
    """Initial state of tests/fixtures/hydro_matrix.c on the active zones [k][j][i][6]; the sixth column is zero without a scalar"""
    a, b, c = root_indices(nx, level, disp)
    d = 1.0 + 0.125 * ((a + 2 * b + 3 * c) % 5).astype(np.float64)
    p = 1.0 + 0.1 * ((2 * a + b + c) % 3).astype(np.float64)
    v = [0.05 * (((3 * a + 5 * b + 7 * c) % 5).astype(np.float64) - 2.0),
         0.04 * (((a + 2 * b + 3 * c) % 7).astype(np.float64) - 3.0),
         0.03 * (((2 * a + b + 4 * c) % 3).astype(np.float64) - 1.0)]
    vac = near_vacuum(a, b, c)
    d = np.where(vac, dvac * d, d)
    p = np.where(vac, pvac * p, p)
    for ax, q in enumerate(boosts(a, b, c)):
        v[ax] = v[ax] + VB[ax] * q
    U = np.zeros(d.shape + (6,))
    U[..., 0] = d; U[..., 1] = d * v[0]; U[..., 2] = d * v[1]; U[..., 3] = d * v[2]
    U[..., 4] = p / (gamma - 1.0) + 0.5 * d * (v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    if nscal:
        U[..., 5] = d * concentration(a, b, c)
    return U


def supersonic_fraction(nx):
    """share of the zones inside blocks boosted by a full +-VB along at least one axis"""
    q = boosts(*root_indices(nx))
    return float(((np.abs(q[0]) == 1.0) | (np.abs(q[1]) == 1.0) | (np.abs(q[2]) == 1.0)).mean())


# fixture tag -> (reference configuration, integrator, order, cour_no, dvac, pvac).  CTU on parabolae is at the brink at the common
# contrast: four of the oracle's six 1-ulp twins of its 24x20x16 run end in NaN; at 0.05 / 0.02 none does and the census still holds
CFG = {"ctu": ("blast", "ctu", 2, 0.4, DVAC, PVAC), "noh": ("blast_noh", "ctu-noh", 2, 0.4, DVAC, PVAC),
       "vl": ("blast_vl", "vl", 2, 0.4, DVAC, PVAC_FLOOR), "ppm": ("blast_ppm", "ctu", 3, 0.4, 0.05, 0.02),
       "vlppm": ("blast_vl_ppm", "vl", 3, 0.4, DVAC, PVAC)}
SHAPES_3D = ((24, 20, 16), (67, 10, 9))
SHAPES_2D = ((67, 35), (24, 20))
CFG_2D = ("ctu", "noh", "vl")
# refined cases: (root zones, [(level, zones, displacement in zones of that level)]).  Every side of a child lies on a block edge
# across which the flow recedes -- the HLLE faces stay on those edges for the three steps, a fan does not spread past a zone --
# and spans blocks of every kind: the fluxes kept on it for the flux correction come from upwind, HLLE and Roe faces
SMR_3D = ((24, 20, 16), [(1, (24, 12, 12), (12, 12, 6))])
SMR_2D = ((48, 36, 1), [(1, (48, 48, 1), (12, 12, 0)), (2, (48, 24, 1), (48, 48, 0))])
# (tag -> reference configuration, integrator, case, cour_no, dvac, pvac.  At the deck's contrast the 3-D refined CTU run meets
#  negative face pressures in its third step -- NaN etas, whose MAX chains no two builds of the reference order alike -- so that
#  case runs at a fifth of the contrast.)
#  The nested van Leer run keeps the positive pressure factor: with E below the kinetic energy in the near-vacuum blocks the
#  REFERENCE's own 1-ulp twins of it (the problem file's `seed` key) part by 3.8e-9 ... 1.4e-7 in a few zones at a child's side --
#  a decision taken on the sign of a floored pressure's rounding noise -- where they part by 2.7e-15 with it; on one level the
#  same blocks leave the twins at 2.7e-15, so the pressure floor is pinned by the single-level van Leer runs.  The golden script
#  records the reference's twins of every nested run; test_oracle_golden.py asserts them.)
SMR_CFG = {"3d_ctu": ("blast_smr", "ctu", SMR_3D, 0.4, 0.1, 0.05), "2d_ctu": ("blast_smr", "ctu", SMR_2D, 0.4, DVAC, PVAC),
           "2d_vl": ("blast_smr_vl", "vl", SMR_2D, 0.4, DVAC, PVAC),
           "2d_vl_floor": ("blast_smr_vl", "vl", SMR_2D, 0.4, DVAC, PVAC_FLOOR)}
# the nested van Leer run WITH the floored pressure: its own twins part (above), so only the strict build -- which has to follow the
# reference decision for decision -- is held to it: the pressure floor at a level boundary, in prolongation and flux correction
STRICT_ONLY = ("2d_vl_floor",)
REF_TWIN_SEEDS = (1, 2, 3, 4, 5, 6)


def gamma(nx3):
    """gamma of the deck the runs of a Grid nx3 zones deep use (decks/athinput.blast, or blast2d for Nx3 = 1: the reference's two decks
    round 5/3 differently)"""
    import importlib
    import os
    aa = importlib.import_module("atmospheric-athena_amd")
    return aa.config.load(os.path.join(orc.DECKS, "athinput.blast2d" if nx3 == 1 else "athinput.blast"), None, "blast").gamma


def overrides(nx, cour_no=0.4):
    return [f"domain1/Nx{d + 1}={int(nx[d])}" for d in range(3)] + [f"time/cour_no={cour_no}"]


def smr_overrides(case, cour_no=0.4):
    root, kids = case
    o = [f"job/num_domains={1 + len(kids)}"] + [f"domain1/Nx{d + 1}={root[d]}" for d in range(3)]
    for n, (lev, nx, disp) in enumerate(kids, 2):
        o += [f"domain{n}/level={lev}"] + [f"domain{n}/Nx{d + 1}={nx[d]}" for d in range(3)]
        o += [f"domain{n}/{k}Disp={disp[d]}" for d, k in enumerate("ijk")]
    return o + [f"time/cour_no={cour_no}"]


def make_sim(cfg, nx, nscal=0):
    """The oracle set up like the reference configuration CFG[cfg] built on tests/fixtures/hydro_matrix.c: blast deck, periodic"""
    _, integrator, order, cour, dvac, pvac = CFG[cfg]
    s = orc.make_sim("blast", overrides(nx, cour), integrator=integrator, order=order, nscal=nscal)
    s.active[...] = pattern(nx, s.grid.run.gamma, dvac=dvac, pvac=pvac, nscal=nscal)
    return s


def make_mesh(tag, nscal=0):
    """The oracle's nested levels (3-D only) set up like the reference's blast_smr configuration on the problem file"""
    _, integrator, case, cour, dvac, pvac = SMR_CFG[tag]
    m = orc.make_mesh("blast", None, smr_overrides(case, cour), integrator=integrator, nscal=nscal)
    for s in m.lev:
        g = s.grid
        s.active[...] = pattern(g.Nx, g.run.gamma, g.level, g.disp if g.level else (0, 0, 0), dvac, pvac, nscal)
    return m


# ---- the fixtures ----------------------------------------------------------------------------------------------------
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCAL_CFG = tuple(CFG)        # the single-level configurations with a scalar fixture on both SHAPES_3D
SCAL_SMR = ("3d_ctu",)       # the nested cases with one


def fixture_name(cfg, nx, nscal=0):
    return ("hydromatrix_s1_" if nscal else "hydromatrix_") + cfg + "_" + "x".join(str(n) for n in (nx if nx[2] > 1 else nx[:2])) + f"_n{NSTEP}"


def smr_fixture_name(tag, nscal=0):
    return ("hydromatrix_s1_smr_" if nscal else "hydromatrix_smr_") + tag + f"_n{NSTEP}"


def load(name):
    """-> a fixture as a dict of arrays.  A scalar fixture (hydromatrix_s1_*: s0, s -- or s0_<l>, s_<l> per level -- and the name of
    its base) comes back as its base's entries with U0 / U (U0_<l> / U_<l>) widened to six columns and nscal = 1"""
    z = np.load(os.path.join(GOLD, name + ".npz"))
    g = {k: z[k] for k in z.files}
    if "base" not in g:
        g.setdefault("nscal", np.array(0))
        return g
    out = load(str(g["base"]))
    for k, v in g.items():
        head, _, level = k.partition("_")
        if head in ("s0", "s"):
            u = ("U0" if head == "s0" else "U") + ("_" + level if level else "")
            out[u] = np.concatenate([out[u], v[..., None]], axis=-1)
        else:
            out[k] = v
    return out


def face_classes(U, axis, gamma):
    """-> integer array shaped like U[..., 0]: the outcome of the Roe solver on the first-order Riemann problem between every zone
    and its upper neighbour along `axis` (0: x1 ...; periodic): 0 Roe flux, 1 F = Fl, 2 F = Fr, 3 HLLE by u0 <= 0, 4 HLLE by
    p_inter < 0 -- the oracle's own solver, one face at a time through its counters' totals"""
    perm = {0: [0, 1, 2, 3, 4], 1: [0, 2, 3, 1, 4], 2: [0, 3, 1, 2, 4]}[axis]
    Ul = np.ascontiguousarray(U[..., perm]).reshape(-1, 5)
    Ur = np.ascontiguousarray(np.roll(U, -1, axis=2 - axis)[..., perm]).reshape(-1, 5)
    cnt = counters()
    out = np.zeros(len(Ul), dtype=np.int8)
    todo = [np.arange(len(Ul))]
    while todo:                                  # bisect on the counters: a batch with one class needs no further split
        idx = todo.pop()
        cnt[...] = 0
        orc.fluxes(Ul[idx], Ur[idx], np.zeros(len(idx)), gamma, 0)
        got = cnt[:4, 0].copy()
        n = int(got.sum())
        if n == 0:
            continue
        if n == len(idx) and (got > 0).sum() == 1:
            out[idx] = 1 + int(np.argmax(got)); continue
        todo += [idx[:len(idx) // 2], idx[len(idx) // 2:]]
    return out.reshape(U.shape[:-1])


# ---- the oracle's live counters --------------------------------------------------------------------------------------
def counters():
    """-> live numpy view [class][direction] of the oracle's census counters"""
    n = len(CLASSES)
    arr = (C.c_long * (3 * n)).in_dll(orc.lib(), "orc_dbg_class")
    return np.ctypeslib.as_array(arr).reshape(n, 3)


def census(cfg, nx, nstep=NSTEP, nscal=0):
    """-> (counts [step][class][direction] of the oracle's run, the Sim after it)"""
    s = make_sim(cfg, nx, nscal).start()
    cnt = counters()
    out = np.zeros((nstep,) + cnt.shape, dtype=np.int64)
    for n in range(nstep):
        cnt[...] = 0
        s.step()
        out[n] = cnt
    return out, s


def census_mesh(tag, nstep=NSTEP, nscal=0):
    """-> counts [step][class][direction] of the oracle's nested run `tag`, all levels together"""
    m = make_mesh(tag, nscal).start()
    cnt = counters()
    out = np.zeros((nstep,) + cnt.shape, dtype=np.int64)
    for n in range(nstep):
        cnt[...] = 0
        m.step()
        out[n] = cnt
    return out


def floored_zones(U, gamma):
    """number of zones of a state whose pressure Cons1D_to_Prim1D floors (convert_var.c:408: P <= TINY_NUMBER)"""
    P = (gamma - 1.0) * (U[..., 4] - 0.5 * (U[..., 1] ** 2 + U[..., 2] ** 2 + U[..., 3] ** 2) / U[..., 0])
    return int((P <= 1.0e-20).sum())


def required(cfg, nscal=0):
    """the classes a run of configuration `cfg` has to reach MIN_COUNT times per sweep direction and step"""
    return required_for(*CFG[cfg][1:3], CFG[cfg][5], nscal)


def required_for(integrator, order, pvac, nscal=0):
    need = list(ROE) + list(RECON)
    if integrator != "vl":
        need += list(TRACE)                    # (van Leer reconstructs without tracing)
    if integrator == "ctu":
        need += list(HCORR)
    if pvac < 0:
        need.append("pressure floor")
    if order == 3:
        need += list(PPM)
    if nscal:
        need += list(SCALAR)
    return need


def scalar_faces(U, axis, gamma):
    """-> counts (Roe flux, F = Fl, F = Fr, HLLE) of the first-order faces along `axis` of a six-column state across which the
    concentration s / d differs: the faces on which a scalar flux taken from the wrong side would show.  (The scalar flux has one
    rule per exit of the solver; the HLLE fallback's is the same whichever test sent the face there.)"""
    r = U[..., 5] / U[..., 0]
    differ = r != np.roll(r, -1, axis=2 - axis)
    n = np.bincount(face_classes(U[..., :5], axis, gamma)[differ].ravel(), minlength=5)
    return np.array([n[0], n[1], n[2], n[3] + n[4]])


def describe_zone(U0, zone, gamma):
    """the outcome of the Roe solver on the six first-order faces of `zone` [k, j, i] of the state U0 before the first step, as a
    line to print beside a failing comparison: it names the branch of the kernel to look at"""
    names = ("Roe", "F=Fl", "F=Fr", "HLLE u0<=0", "HLLE p_inter<0")
    k, j, i = (int(z) for z in zone)
    out = []
    for ax in range(3 if U0.shape[0] > 1 else 2):
        cls = face_classes(U0[..., :5], ax, gamma)
        lo = [k, j, i]; lo[2 - ax] = (lo[2 - ax] - 1) % U0.shape[2 - ax]
        out.append(f"x{ax + 1} lower {names[cls[tuple(lo)]]}, upper {names[cls[k, j, i]]}")
    return f"zone [k, j, i] = {[k, j, i]}: " + "; ".join(out)
