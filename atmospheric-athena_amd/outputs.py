"""The ``<outputN>`` blocks of a deck: init_output (output.c:171-487) and data_output (:498-569) of the reference for the
dump formats this package writes -- ``hst`` (history.py), ``rst`` (restart.py), ``vtk`` and ``bin`` (dumps.py), the last two
with ``out = cons`` (the default) or ``out = prim``.

Keys read per block: ``out_fmt``, ``out``, ``dt`` (required), ``time`` (default: the current time), ``num`` (default 0),
``level`` / ``domain`` (default -1: all), ``id``, ``dat_fmt``; ``<job>maxout`` says how many blocks are looked at.  Everything
else the reference knows -- single-variable outputs (``out = d``, ``P``, ``V1`` ... with slices), ``out_fmt = tab | ppm | pgm |
pdf``, user outputs by ``name =`` -- is refused by ``from_par`` with the block and the value named: a run must not find out at
its first dump.

``from_par(..., single=True)`` -- off by default -- also reads the single-variable blocks by init_output's rules (output.c:363-471):
``out = d | M1 .. cs2`` (``flux`` with ``usr_expr_flag``), ``id``, ``dat_fmt``, ``dmin / dmax``, the slices of `parse_slice`, ``ndim``,
``out_fmt = vtk | tab | pgm``; `slice_search` / `slice_zones` / `single_ranges` are the index search of OutData1/2, and a target's
``write_single(out, self)`` (driver.Driver: one rank, a 2-D or 3-D Grid) makes the file.  ``ppm``, ``pdf``, ``name =``, ``S``,
particle expressions and ``tab`` dumps stay refused.

``data_output(target, flag)`` drives a *target*: anything with ``time`` and the three writers ``write_dump(out, self)``,
``write_history(out, self)``, ``write_restart(out, self)``: driver.Driver (one Grid per rank), driver.MeshRun (every level of a
refined mesh on one GPU) and driver.MeshDriver (a refined mesh over several ranks).  What the three have in common on this side --
the restart file between header and trailer, the host-block state, the history row, the level / domain test, ``data_output``
and ``main`` -- is written once in their base class driver._Runner.  File names are ath_fname's (dumps.fname); rank r of a
multi-rank run writes under ``id<r>/`` with ``-id<r>`` in the base name for r > 0 (main.c:227-232, :785-850), every rank its own
Grids; the history of a Domain goes out once, under rank 0's directory.

``OutputSet(..., overlap=True)`` writes the ``vtk`` / ``bin`` dumps of targets that have the route beside the run
(``overlapped_dump``: a device snapshot taken when the block fires, its copy to page-locked memory next to the following steps,
the file written by the thread of dumps.OverlapWriter); the files and ``written`` are those of the synchronous run.  One rule:
only the thread that drives the run calls the library -- ``poll`` and ``finish`` belong to it.  ``overlap_rst=True`` -- a switch
of its own -- does the same for the restart dump (``overlapped_restart``: the double-precision payload of every Grid from ONE
snapshot slot per Grid, the file behind the vtk / bin files already queued).

``OutputSet(..., hst_queued=True)`` -- off by default like the two above -- lets `run` keep a target's queued steps going through
the FIRST ``hst`` block: the block is armed on the device for every advance() (``hst_armed``), its rows come back with the call and
are written with their own time and dt.  The files are those of the run with the keyword off.
"""
from __future__ import annotations

import collections
import io
import os
import warnings
from dataclasses import dataclass
from typing import List, Optional

from .athinput import ParError, ParTable

MAXOUT_DEFAULT = 10
DUMPS = ("vtk", "bin")


@dataclass
class Output:
    """OutputS of the reference, the members the dumps use."""
    n: int                      # the N of <outputN>
    out_fmt: str
    out: str                    # "cons" | "prim"
    t: float                    # next output time
    dt: float
    num: int                    # next output number
    level: int = -1
    domain: int = -1
    id: str = ""
    dat_fmt: Optional[str] = None
    # a single-variable output (from_par(single=True)): `out` is the expression; ndim as init_output counts it (output.c:390-411);
    # xl / xu the slice bounds and raw_reduce the reduce_x1/2/3 flags as parse_slice leaves them; sdmin / sdmax: dmin / dmax are set;
    # gmin / gmax: the running pair the writers keep (not in the parameter table: a restarted run begins them again, as the
    # reference's init_output does)
    single: bool = False
    ndim: int = 0
    xl: tuple = (0.0, 0.0, 0.0)
    xu: tuple = (0.0, 0.0, 0.0)
    raw_reduce: tuple = (0, 0, 0)
    sdmin: bool = False
    sdmax: bool = False
    dmin: float = 0.0
    dmax: float = 0.0
    gmin: float = 1.0e20          # HUGE_NUMBER, defs.h.in:161
    gmax: float = -1.0e20

    @property
    def prim(self) -> bool:
        return self.out == "prim"


SINGLE_EXPR = ("d", "M1", "M2", "M3", "E", "V1", "V2", "V3", "P", "cs2")     # getexpr (output.c:1279-1347) for adiabatic hydro
SINGLE_FMT = ("vtk", "tab", "pgm")
_PARTICLE_EXPR = ("dpar", "M1par", "M2par", "M3par", "V1par", "V2par", "V3par")
NGHOST = 4


def _atof(s: str) -> float:
    """atof: the longest numeric prefix, 0.0 where there is none"""
    import re
    m = re.match(r"\s*[-+]?(\d+\.?\d*([eE][-+]?\d+)?|\.\d+([eE][-+]?\d+)?|inf(inity)?|nan)", s, re.I)
    return float(m.group(0)) if m else 0.0


def parse_slice(par: ParTable, block: str, ax: str, l: float, u: float):
    """parse_slice (output.c:1391-1418): ``v`` | ``lo:hi`` | ``:`` | ``lo:`` | ``:hi`` -> (l, u, flag); a missing end keeps the
    root Domain's"""
    if not par.exist(block, ax):
        return l, u, 0
    expr = par.gets(block, ax)
    if ":" in expr:
        a, b = expr.split(":", 1)
        if b.strip():
            u = _atof(b)
        if a.strip():
            l = _atof(a)
    else:
        l = u = _atof(expr)
    if l > u:
        raise ParError(f"[parse_slice]: lower slice limit {l!r} > upper {u!r} in {expr}")
    return l, u, 1


def slice_search(l: float, u: float, minx: float, dx: float, n: int):
    """The index search of OutData1/2 (output.c:763-780 and its siblings) along one direction of `n` active zones from `minx`,
    with fc_pos's face position ``minx + (Real)(k - ks)*dx``: -> (kstart, kend) counted from the first active zone, or None where
    the range misses the Grid (``xu < MinX || xl >= MaxX``, MaxX = MinX + Nx*dx, init_grid.c:111)."""
    if u < minx or l >= minx + float(n) * dx:
        return None
    k = 1
    while l >= minx + float(k) * dx:
        k += 1
    start = k - 1
    k = n - 1
    while u < minx + float(k) * dx:
        k -= 1
    return start, k


def slice_zones(l: float, u: float, minx: float, dx: float, n: int):
    """The zones OutData1/2 SUM for a slice, counted from the first active zone.  The search leaves kstart / kend as indices of the
    Grid's arrays (they begin at kl+1 = ks+1), and the loops then read ``expr(pgrid, i+il, j+jl, k+kl)`` for k = kstart .. kend
    (output.c:789-790): the first active index is added twice, so the zones lie nghost = 4 above the slice's own -- the upper
    slices of a Grid are read from its ghost zones (never past them: kend <= ke).  A direction of one zone has ks = 0: no shift."""
    r = slice_search(l, u, minx, dx, n)
    if r is None:
        return None
    first = NGHOST if n > 1 else 0
    return r[0] + first, r[1] + first


def single_ranges(out: Output, Nx, minx, dx):
    """What OutData1/2/3 do for the block `out` on a Grid of Nx zones: -> (reduce, lo, hi) for lib.Grid.outdata /
    dumps.outdata_from_values -- reduce[a]: direction a is summed over the zones lo[a] .. hi[a] (slice_zones) --, or None where
    the slice misses the Grid (no file).  A 2-D Grid's output of ndim 2 is the Grid itself (output.c:748-757)."""
    gdim = sum(1 for v in Nx if v > 1)
    red, lo, hi = [0, 0, 0], [0, 0, 0], [0, 0, 0]
    if out.ndim == gdim:
        return tuple(red), tuple(lo), tuple(hi)
    rr = out.raw_reduce
    if out.ndim == 2:                       # OutData2 on a 3-D Grid: x3, else x2, else x1
        which = [2 if rr[2] else 1 if rr[1] else 0]
    elif not rr[0]:                         # OutData1: the kept direction is the first that is not reduced
        which = [2, 1]
    elif not rr[1]:
        which = [2, 0]
    else:
        which = [1, 0]
    for a in which:
        if u_misses(out.xl[a], out.xu[a], minx[a], dx[a], Nx[a]):
            return None
    for a in which:
        red[a] = 1
        if Nx[a] == 1:                      # output.c:947-949: kstart = kl, kend = ku
            continue
        lo[a], hi[a] = slice_zones(out.xl[a], out.xu[a], minx[a], dx[a], Nx[a])
    return tuple(red), tuple(lo), tuple(hi)


def u_misses(l, u, minx, dx, n) -> bool:
    return u < minx or l >= minx + float(n) * dx


def payload_shape(reduce, Nx):
    """the dimensions of the array the writers get, slowest first: the kept directions of more than one zone"""
    return tuple(Nx[a] for a in (2, 1, 0) if not reduce[a] and Nx[a] > 1)


class OutputSet:
    def __init__(self, par: ParTable, outs: List[Output], rst: Optional[Output], rundir: str, rank: int, nranks: int,
                 rst_ngrid=None, rst_mesh_ngrid=None, rst_mesh_nproc=None, overlap: bool = False, overlap_max_bytes: int = 8 << 30,
                 overlap_rst: bool = False, hst_queued: bool = False):
        """overlap = True: vtk / bin dumps of targets that have the route (see `overlapped_dump`) are written beside the run;
        overlap_max_bytes: the largest payload that may take it (each Grid that dumps keeps two device buffers and two
        page-locked buffers of its payload's size).  overlap_rst = True, independent of `overlap`: the restart dump too (see
        `overlapped_restart`; one device buffer and one page-locked buffer of the restart payload per Grid, under the same cap).
        hst_queued = True, a switch of its own: `run` leaves the first ``hst`` block out of the stop times of a target whose
        steps queue on the device and takes its rows from there (`hst_armed`; the same files)."""
        self.par, self.outs, self.rst = par, outs, rst
        self.hst_queued = bool(hst_queued)
        self.single = False                   # from_par(single=True): single-variable blocks may stand in `outs`
        self._single_checked = False
        self.overlap, self.overlap_max_bytes = bool(overlap), int(overlap_max_bytes)
        self.overlap_rst = bool(overlap_rst)
        self._writer = None                   # dumps.OverlapWriter, made by the first overlapped dump
        self._pending = collections.deque()   # snapshots taken whose payload is still on its way: jobs in the order of `written`
        self._inflight = []                   # jobs the writer has, their slots not yet given back
        self._warned = set()                  # fall-backs to the synchronous path already told
        self.rst_ngrid = tuple(int(v) for v in rst_ngrid) if rst_ngrid else None      # restart dumps cut for other Grids
        # ... of a refined mesh: NGrid of every Domain, level by level (restart.domain_blocks), and the ranks they are dealt to
        self.rst_mesh_ngrid = [tuple(int(v) for v in g) for g in rst_mesh_ngrid] if rst_mesh_ngrid else None
        self.rst_mesh_nproc = rst_mesh_nproc
        if self.rst_mesh_ngrid and rst_mesh_nproc is None:
            from . import restart
            self.rst_mesh_nproc = restart.mesh_nproc(self.rst_mesh_ngrid)
        self.rank, self.nranks = rank, nranks
        self.basename = par.gets("job", "problem_id")
        self.dir = os.path.join(rundir, f"id{rank}") if nranks > 1 else rundir
        self.written: List[str] = []          # relative to `dir`, in the order of writing

    @classmethod
    def from_par(cls, par: ParTable, time: float = 0.0, rundir: str = ".", rank: int = 0, nranks: int = 1,
                 rst_ngrid=None, rst_mesh_ngrid=None, rst_mesh_nproc=None, overlap: bool = False,
                 overlap_max_bytes: int = 8 << 30, overlap_rst: bool = False, hst_queued: bool = False,
                 single: bool = False, problem: Optional[str] = None) -> "OutputSet":
        """init_output.  single = True -- off by default: nothing changes without it -- also takes the single-variable blocks
        (``out = d | M1 | M2 | M3 | E | V1 | V2 | V3 | P | cs2`` with ``id``, ``x1 / x2 / x3`` slices, ``dmin / dmax``, ``dat_fmt``,
        ``out_fmt = vtk | tab | pgm``; ``out = flux`` with ``usr_expr_flag = 1`` for a problem whose file defines it -- `problem`, or
        the target's at the first output) by init_output's rules (output.c:363-471); one rank, a 2-D or 3-D Grid, synchronous.

        Like the reference it completes the parameter table (defaults of the blocks it reads; for rank
        r > 0 ``<job>problem_id`` gains ``-id<r>``, main.c:227-232): the table is what a restart dump carries.
        rst_ngrid = (n1, n2, n3): a one-rank run writes its restart dumps as the n1 x n2 x n3 ranks of the reference would, one
        file per Grid under ``id<r>/`` (Driver.write_restart; x1 cuts are written and read, never run).
        rst_mesh_ngrid = [(n1, n2, n3) for <domain1>, <domain2>, ...]: the same for a refined mesh on one process (MeshRun, or
        MeshDriver on one rank): one file per RANK of the reference's MPI run on those cuts, each with the Grids the reference
        deals to that rank (restart.mesh_grid_boxes).  rst_mesh_nproc: the number of those ranks; by default the smallest that
        the rules allow (restart.mesh_nproc) -- a larger one leaves ranks without a Grid of the root."""
        if rst_ngrid is not None:
            if nranks > 1:
                raise ValueError("[init_output]: rst_ngrid takes a one-rank run")
            if len(tuple(rst_ngrid)) != 3 or min(int(v) for v in rst_ngrid) < 1:
                raise ValueError(f"[init_output]: rst_ngrid = {rst_ngrid!r} (three counts >= 1)")
            if par.geti("domain1", "Nx2") == 1 and par.geti("domain1", "Nx3") == 1:
                raise ValueError("[init_output]: rst_ngrid is not built for a 1-D Grid (Nx2 = Nx3 = 1): it is one Grid on one rank")
        if rst_mesh_ngrid is None and rst_mesh_nproc is not None:
            raise ValueError("[init_output]: rst_mesh_nproc without rst_mesh_ngrid")
        if rst_mesh_ngrid is not None:
            from . import restart
            if rst_ngrid is not None:
                raise ValueError("[init_output]: rst_ngrid (a single-level run) and rst_mesh_ngrid (a refined mesh) together")
            if nranks > 1:
                raise ValueError("[init_output]: rst_mesh_ngrid takes a one-rank run")
            if par.geti("domain1", "Nx3") == 1:
                raise ValueError("[init_output]: rst_mesh_ngrid is not built for a 2-D mesh (Nx3 = 1), nor for a 1-D run")
            blocks = restart.domain_blocks(par)
            given = [tuple(g) for g in rst_mesh_ngrid]
            if len(given) != len(blocks) or any(len(g) != 3 or min(int(v) for v in g) < 1 for g in given):
                raise ValueError(f"[init_output]: rst_mesh_ngrid = {rst_mesh_ngrid!r} (three counts >= 1 for each of the "
                                 f"{len(blocks)} <domainN> blocks)")
            rst_mesh_ngrid = [given[n - 1] for n in blocks]                # level by level, as the reference visits them
            rst_mesh_nproc = restart.mesh_nproc(rst_mesh_ngrid, rst_mesh_nproc)      # (ValueError: Grids no such rank count divides)
        if single:
            if nranks > 1:
                raise ValueError("[init_output]: single = True takes a one-rank run (several ranks would each hold a part of a slice)")
            if par.geti("domain1", "Nx2") == 1 and par.geti("domain1", "Nx3") == 1:
                raise ValueError("[init_output]: single = True is not built for a 1-D Grid (Nx2 = Nx3 = 1)")
        if nranks > 1 and rank != 0:
            par.blocks["job"]["problem_id"] = "%s-id%d" % (par.gets("job", "problem_id"), rank)
        maxout = par.geti_def("job", "maxout", MAXOUT_DEFAULT)
        outs: List[Output] = []
        rst = None
        for n in range(1, maxout + 1):
            block = f"output{n}"
            if not par.exist(block, "out_fmt") and not par.exist(block, "name"):
                warnings.warn(f"[init_output]: neither {block}/out_fmt, nor {block}/name exist")      # output.c:195-199: not fatal
                continue
            if par.exist(block, "name"):
                raise ParError(f"[init_output]: <{block}> name = {par.gets(block, 'name')}: user-defined outputs are not built")
            fmt = par.gets(block, "out_fmt")
            out = par.gets(block, "out") if par.exist(block, "out") else "cons"
            if single and out not in ("cons", "prim"):
                if overlap:
                    raise ValueError(f"[init_output]: <{block}> out = {out}: single-variable outputs are written synchronously; "
                                     "single = True does not go with overlap = True")
                outs.append(cls._single_block(par, n, block, fmt, out, time, problem))
                continue
            if out not in ("cons", "prim"):
                raise ParError(f"[init_output]: <{block}> out = {out} (out_fmt = {fmt}): single-variable outputs are not built; "
                               "dumps take out = cons or out = prim")
            ok = ("hst", "rst", "vtk", "bin") if out == "cons" else DUMPS
            if fmt not in ok:
                raise ParError(f"[init_output]: Unsupported dump mode for {block}/out_fmt={fmt} for out={out} "
                               f"(built: {', '.join(ok)})")
            o = Output(n=n, out_fmt=fmt, out=out,
                       t=par.getd_def(block, "time", time), num=par.geti_def(block, "num", 0), dt=par.getd(block, "dt"),
                       level=par.geti_def(block, "level", -1), domain=par.geti_def(block, "domain", -1),
                       id=par.gets(block, "id") if par.exist(block, "id") else f"out{n}",
                       dat_fmt=par.gets(block, "dat_fmt") if par.exist(block, "dat_fmt") else None)
            par.blocks[block].setdefault("id", o.id)
            par.blocks[block].setdefault("out", out)
            if fmt == "rst":
                rst = o                         # output.c:299-305: kept apart, one per run (the last one named wins)
            else:
                outs.append(o)
        self = cls(par, outs, rst, rundir, rank, nranks, rst_ngrid, rst_mesh_ngrid, rst_mesh_nproc, overlap, overlap_max_bytes,
                   overlap_rst, hst_queued)
        self.single = bool(single)
        return self

    @staticmethod
    def _single_block(par: ParTable, n: int, block: str, fmt: str, out: str, time: float, problem: Optional[str]) -> Output:
        """output.c:363-471 for one block whose `out` is neither cons nor prim"""
        usr = par.geti(block, "usr_expr_flag") if par.exist(block, "usr_expr_flag") else 0
        if usr:                                 # get_usr_expr: prob/ioniz_sphere.c:241-249 knows "flux" and nothing else
            if out != "flux":
                raise ParError(f"[init_output]: <{block}> usr_expr_flag = {usr}, out = {out}: the only user expression built is "
                               "out = flux (the EdgeFlux of ioniz_sphere)")
            if problem is not None and problem != "ioniz_sphere":
                raise ParError(f"[init_output]: <{block}> out = flux: problem \"{problem}\" defines no such expression (ioniz_sphere does)")
        elif out == "S":
            raise ParError(f"[init_output]: <{block}> out = S: the entropy calls pow(), whose device version is not the host's to the "
                           "last bit; it is not built")
        elif out in _PARTICLE_EXPR:
            raise ParError(f"[init_output]: <{block}> out = {out}: particle expressions are not built")
        elif out not in SINGLE_EXPR:
            raise ParError(f"[init_output]: <{block}> out = {out}: Unknown data expression (built: {', '.join(SINGLE_EXPR)}; "
                           "flux with usr_expr_flag = 1)")
        if fmt in ("ppm", "pdf"):
            why = ("the palette tables are the reference's program text and are not copied" if fmt == "ppm"
                   else "probability distributions are not built")
            raise ParError(f"[init_output]: <{block}> out_fmt = {fmt} (out = {out}): {why}")
        if fmt not in SINGLE_FMT:
            raise ParError(f"[init_output]: Unsupported {block}/out_fmt={fmt} (built for out = {out}: {', '.join(SINGLE_FMT)})")
        Nx = [par.geti("domain1", f"Nx{a + 1}") for a in range(3)]
        ndim = 1 + sum(1 for a in (1, 2) if Nx[a] > 1)
        xl, xu, rr = [], [], []
        for a in range(3):
            l, u, f = parse_slice(par, block, f"x{a + 1}", par.getd("domain1", f"x{a + 1}min"), par.getd("domain1", f"x{a + 1}max"))
            xl.append(l); xu.append(u); rr.append(f)
            if f and (a == 0 or Nx[a] > 1):
                ndim -= 1
        if ndim <= 0:
            raise ParError(f"Too many slices specified in {block}")
        if fmt == "vtk" and ndim == 1:
            raise ParError(f"[output_vtk]: <{block}> is 1-D: Only able to output 2D or 3D")
        if fmt == "pgm" and ndim != 2:
            raise ParError(f"[output_pgm]: <{block}> is {ndim}-D: Output must be a 2D slice")
        o = Output(n=n, out_fmt=fmt, out=out,
                   t=par.getd_def(block, "time", time), num=par.geti_def(block, "num", 0), dt=par.getd(block, "dt"),
                   level=par.geti_def(block, "level", -1), domain=par.geti_def(block, "domain", -1),
                   id=par.gets(block, "id") if par.exist(block, "id") else f"out{n}",
                   dat_fmt=par.gets(block, "dat_fmt") if par.exist(block, "dat_fmt") else None,
                   single=True, ndim=ndim, xl=tuple(xl), xu=tuple(xu), raw_reduce=tuple(rr),
                   sdmin=par.exist(block, "dmin"), sdmax=par.exist(block, "dmax"),
                   dmin=par.getd(block, "dmin") if par.exist(block, "dmin") else 0.0,
                   dmax=par.getd(block, "dmax") if par.exist(block, "dmax") else 0.0)
        par.blocks[block].setdefault("id", o.id)
        par.blocks[block].setdefault("out", out)
        return o

    def data_output(self, target, flag: int, settled: Optional[Output] = None) -> None:
        """flag = 1 writes every output; flag = 0 those whose next time has passed.  A block that fires advances by its dt
        ONCE (output.c:509-512).  The restart dump goes first, after every block's next number and time have been written
        back into the parameter table (:526-543), so that a restarted run continues the numbering.  With overlapped dumps it
        begins with a `poll`: the payloads that have arrived go to the writer, the files that are complete give their slots back.
        settled: a block whose row for this time is already written and counted (`run` with hst_queued: the device has
        applied the rule behind this step, t += dt and num += 1 are done) -- it is not asked again."""
        self.poll()
        if not self._single_checked and any(o.single for o in self.outs):
            # before the first file: a target without the route refuses the keyword (``single_route()`` -> None or the reason)
            why = target.single_route(self) if hasattr(target, "single_route") else "this target writes no single-variable outputs"
            if why is not None:
                raise ValueError(f"[data_output]: single = True: {why}")
            self._single_checked = True
        time = target.time
        fire = []
        for o in self.outs:
            f = bool(flag)
            if o is settled:
                pass
            elif time >= o.t:
                o.t += o.dt
                f = True
            fire.append(f)
        r = self.rst
        if r is not None:
            f = bool(flag)
            if time >= r.t:
                r.t += r.dt
                f = True
            if f:
                for o, fo in zip(self.outs, fire):
                    b = self.par.blocks[f"output{o.n}"]
                    b["num"] = "%d" % (o.num + 1 if fo else o.num)
                    b["time"] = "%.15e" % o.t
                b = self.par.blocks[f"output{r.n}"]
                b["num"] = "%d" % (r.num + 1)
                b["time"] = "%.15e" % r.t
                target.write_restart(r, self)
                r.num += 1
        for o, fo in zip(self.outs, fire):
            if fo:
                if o.out_fmt == "hst":
                    target.write_history(o, self)
                elif o.single:              # (a slice that misses the Grid writes nothing; the number advances all the same)
                    target.write_single(o, self)
                else:
                    target.write_dump(o, self)
                o.num += 1

    def path(self, rel: str) -> str:
        """The place of a file named relative to this rank's run directory; remembers it in `written`."""
        p = os.path.join(self.dir, rel)
        os.makedirs(os.path.dirname(p) or ".", exist_ok=True)
        self.written.append(rel)
        return p


    # ---- overlapped vtk / bin dumps: device snapshot, background write (dumps.OverlapWriter) -----------------------------------
    def overlap_fallback(self, kind: str, reason: str, switch: str = "overlap") -> None:
        """a dump of a run with overlap = True (or overlap_rst = True: `switch`) takes the synchronous path: said once per kind
        of reason and switch"""
        if (switch, kind) not in self._warned:
            self._warned.add((switch, kind))
            warnings.warn(f"[data_output]: {switch} = True, but {reason}: these dumps are written synchronously (the same files)")

    # ---- history rows from the device (hst_queued; csrc/run.hip aa_run_hst_arm) ----------------------------------------------------
    def hst_armed(self, target) -> Optional[Output]:
        """The block `run` arms on the device for the next advance of `target`, or None: hst_queued on, the FIRST ``hst`` block
        (further ones stay stop times), and a target with the route -- ``hst_route()`` -> None, ``advance(..., hst=)`` and
        ``write_history_rows(out, self)``: driver.Driver on one rank with a 2-D / 3-D Grid on a device, driver.MeshRun.  Every
        other target keeps today's path, and the first case of a kind has warned (as `overlap_fallback` does)."""
        if not self.hst_queued:
            return None
        o = next((o for o in self.outs if o.out_fmt == "hst"), None)
        if o is None:
            return None
        why = target.hst_route() if hasattr(target, "hst_route") else ("engine", "this engine keeps no state on a device")
        if why is not None:
            if ("hst_queued", why[0]) not in self._warned:
                self._warned.add(("hst_queued", why[0]))
                warnings.warn(f"[data_output]: hst_queued = True, but {why[1]}: the history block stays a stop time of the run "
                              "(the same files)")
            return None
        return o

    def overlapped_dump(self, source, rel: str, fmt, prim: bool, level=None, domain: int = 0, time=None, dt=None) -> bool:
        """The overlapped route of a target's write_dump for the dump `rel` (relative to this rank's directory) of `source`:
        something with ``dump_snapshot(fmt, prim, max_bytes)`` -> a snapshot (``ready()``, ``wait()``, ``sections()``,
        ``release()``), ``dump_snapshot_bytes(fmt)``, ``dump_geometry(prim, level, domain, time, dt)``, ``DUMP_SLOTS`` and
        ``composite`` -- lib.Grid.  -> False when the route does not exist here (overlap off; no such source; a Grid cut into slabs;
        a payload beyond overlap_max_bytes): the caller then writes synchronously, and the first such case of a kind has warned.

        Else the snapshot is queued NOW, behind what the last step launched -- the file will hold this instant's state -- and
        `rel` enters `written` now, as the synchronous run would have it; the header is made now too, from the time and dt of now.
        Nothing waits: the copy to the host runs beside the next step, `poll` (every data_output begins with one) hands payloads
        that have arrived to the writer thread and gives the slots of finished files back.  Every HIP call stays on this thread.

        A source has DUMP_SLOTS (two) slots.  When all are held -- the dumps come faster than copy and file write take -- this
        call WAITS for the source's oldest file to be complete: the synchronous cost reappears, one dump late."""
        if not self.overlap:
            return False
        if source is None or not hasattr(source, "dump_snapshot"):
            self.overlap_fallback("engine", "this engine keeps no state on a device")
            return False
        if getattr(source, "composite", False):
            self.overlap_fallback("slabs", "a Grid cut into slabs inside the library takes no snapshot (aa_dump_section is the path there)")
            return False
        if getattr(source, "ndim", 3) == 1:
            self.overlap_fallback("1-D", "a 1-D Grid takes no snapshot (its dumps are a few kilobytes)")
            return False
        nbytes = int(source.dump_snapshot_bytes(fmt))
        if nbytes > self.overlap_max_bytes:
            self.overlap_fallback("max_bytes", f"a payload of {nbytes} bytes is beyond overlap_max_bytes = {self.overlap_max_bytes}")
            return False
        from . import dumps
        slots = int(getattr(source, "DUMP_SLOTS", 2))
        while self._held(source, "dump") >= slots:
            self._wait_oldest(source, "dump")
        snap = source.dump_snapshot(fmt, prim, self.overlap_max_bytes)
        try:
            header, titles = dumps.dump_head(fmt, **source.dump_geometry(prim, level, domain, time, dt))
            path = self.path(rel)
        except BaseException:
            snap.release()
            raise
        self._pending.append({"kind": "dump", "sources": (source,), "snaps": [snap], "path": path, "header": header,
                              "titles": titles, "trailer": b"", "ticket": None})
        return True

    def overlapped_restart(self, sources, rel: str, nstep: int, time: float, dt: float) -> bool:
        """The overlapped route of a target's write_restart for the file `rel` holding the Grids `sources`, root first: each
        something with ``rst_snapshot(max_bytes)`` -> a snapshot (``ready()``, ``wait()``, ``sections()`` -> [(label, float64
        array)], ``release()``), ``rst_snapshot_bytes()``, ``RST_SLOTS`` and ``composite`` -- lib.Grid.  -> False when the route
        does not exist here (overlap_rst off; no such source; a Grid cut into slabs; a payload beyond overlap_max_bytes): the
        caller then writes synchronously, and the first such case of a kind has warned.

        Else everything dump_restart does in front of the payload happens NOW, on this thread: the time and the step count go
        into the parameter table (restart.c:522-523), the table is serialised with N_STEP / TIME / TIME_STEP into the file's
        header bytes -- the next data_output changes the table again --, `rel` enters `written`, and every source's snapshot is
        queued behind what the last step launched.  ONE job holds the snapshots of all sources; it is ready when all are, and it
        stands behind the vtk / bin jobs already pending: files reach the writer in the order of `written`.  The trailer is
        restart.write_trailer's.

        A source has RST_SLOTS (one) slot.  While it is held -- the restart dumps come faster than copy and file write take --
        this call WAITS for that source's oldest restart file to be complete."""
        if not self.overlap_rst:
            return False
        sources = list(sources) if sources is not None else []
        if not sources or any(s is None or not hasattr(s, "rst_snapshot") for s in sources):
            self.overlap_fallback("engine", "this engine keeps no state on a device", "overlap_rst")
            return False
        if any(getattr(s, "composite", False) for s in sources):
            self.overlap_fallback("slabs", "a Grid cut into slabs inside the library takes no snapshot (aa_rst_section_get is the "
                                  "path there)", "overlap_rst")
            return False
        if any(getattr(s, "ndim", 3) == 1 for s in sources):
            self.overlap_fallback("1-D", "a 1-D Grid takes no snapshot (its dumps are a few kilobytes)", "overlap_rst")
            return False
        nbytes = max(int(s.rst_snapshot_bytes()) for s in sources)
        if nbytes > self.overlap_max_bytes:
            self.overlap_fallback("max_bytes", f"a restart payload of {nbytes} bytes is beyond overlap_max_bytes = "
                                  f"{self.overlap_max_bytes}", "overlap_rst")
            return False
        from . import restart
        for s in sources:
            while self._held(s, "rst") >= int(getattr(s, "RST_SLOTS", 1)):
                self._wait_oldest(s, "rst")
        par = self.par
        par.blocks.setdefault("time", {})["time"] = "%e" % time
        par.blocks["time"]["nstep"] = "%d" % nstep
        head, tail = io.BytesIO(), io.BytesIO()
        restart.write_header(head, restart.par_dump(par), nstep, time, dt)
        restart.write_trailer(tail)
        snaps = []
        try:
            for s in sources:
                snaps.append(s.rst_snapshot(self.overlap_max_bytes))
            path = self.path(rel)
        except BaseException:
            for sn in snaps:
                sn.release()
            raise
        self._pending.append({"kind": "rst", "sources": tuple(sources), "snaps": snaps, "path": path, "header": head.getvalue(),
                              "titles": None, "trailer": tail.getvalue(), "ticket": None})
        return True

    def _held(self, source, kind: str) -> int:
        """slots of `source` that jobs of this kind hold: snapshots on their way and files the writer has"""
        return sum(1 for j in list(self._pending) + self._inflight
                   if j["kind"] == kind and any(s is source for s in j["sources"]))

    def _submit(self, job) -> None:
        from . import dumps
        if self._writer is None:
            self._writer = dumps.OverlapWriter()
        self._inflight.append(job)

        def on_done(job=job):                     # (run by poll / wait / finish on the driving thread: release calls HIP)
            self._inflight.remove(job)
            for sn in job["snaps"]:
                sn.release()
        if job["kind"] == "rst":                  # every Grid's labelled sections, root first (restart.write_grid_sections' bytes)
            from . import restart
            pairs = [p for sn in job["snaps"] for p in sn.sections()]
            titles, sections = [restart._tag(label) for label, _ in pairs], [a for _, a in pairs]
        else:
            titles, sections = job["titles"], job["snaps"][0].sections()
        job["ticket"] = self._writer.submit(job["path"], job["header"], titles, sections, on_done, job["trailer"])

    def _wait_oldest(self, source, kind: str) -> None:
        """blocks until the oldest job of this kind of `source` is on disk and its slot free (files are written in the order of
        `written`: everything taken before it goes to the writer first)"""
        def mine(j): return j["kind"] == kind and any(s is source for s in j["sources"])
        held = [j for j in self._inflight if mine(j)]
        if not held:
            while self._pending:
                j = self._pending.popleft()
                for sn in j["snaps"]:
                    sn.wait()
                self._submit(j)
                if mine(j):
                    held = [j]
                    break
        self._writer.wait(held[0]["ticket"])

    def poll(self) -> None:
        """Never blocks: one event query per pending snapshot (oldest first, up to the first that is still in flight); hands the
        ones on the host to the writer, releases the slots of the files that are complete, re-raises what the writer met."""
        while self._pending and all(sn.ready() for sn in self._pending[0]["snaps"]):
            self._submit(self._pending.popleft())
        if self._writer is not None:
            self._writer.poll()

    def finish(self) -> None:
        """Waits for the snapshots still in flight, hands them to the writer, joins it and re-raises what it met: afterwards every
        file in `written` is on disk and every slot free.  May be called again."""
        try:
            while self._pending:
                for sn in self._pending[0]["snaps"]:
                    sn.wait()
                self._submit(self._pending.popleft())
        finally:
            if self._writer is not None:
                self._writer.finish()


def run(target, outputs: OutputSet, tlim: float, nlim: int = -1) -> None:
    """main() of the reference around the loop: forced output after the start (main.c:501; a restarted run -- a target with
    ``restarted`` set -- skips it), data_output(0) at the top of every pass (:524), forced output after the loop (:743).
    `target`: start(), step(), time, nstep and the writers.  A target that also has ``advance(t_stop, nstep_stop)`` and whose
    ``may_batch()`` says so (driver.Driver on a 1-D Grid) takes every stretch between two output times in ONE call: up to the
    earliest next time of any block, or tlim.  data_output(0) writes nothing between those times, so the files are the same.

    With ``OutputSet(hst_queued=True)`` the first ``hst`` block of such a target (`OutputSet.hst_armed`) is no stop time: its
    t, dt and nlim go along with advance(), which applies data_output's rule for that block behind every step it takes
    (csrc/time_step.h hst_row_due) and makes the rows where they are due.  Each row that comes back is written with its own time
    and dt and counted -- t += dt, num += 1 -- before the next data_output(0), which does not ask that block again for the step
    the call ended on: a restart dump fired there carries the table the per-step run writes."""
    batch = hasattr(target, "advance") and hasattr(target, "may_batch")
    armed = getattr(outputs, "hst_armed", None)
    try:
        target.start()
        if not getattr(target, "restarted", False):
            outputs.data_output(target, 1)
        settled = None
        while target.time < tlim and (nlim < 0 or target.nstep < nlim):
            if settled is not None:
                outputs.data_output(target, 0, settled)
            else:
                outputs.data_output(target, 0)
            done, settled = 0, None
            if batch and target.may_batch():      # (asked on every pass: zones pinned since the last one end the batching)
                h = armed(target) if armed is not None else None
                t_stop = min([tlim] + [o.t for o in outputs.outs if o is not h] + ([outputs.rst.t] if outputs.rst is not None else []))
                if t_stop > target.time:          # (a block whose next time has already passed fires again on the next pass)
                    if h is None:
                        done = target.advance(t_stop, nlim if nlim >= 0 else None)
                    else:
                        done = target.advance(t_stop, nlim if nlim >= 0 else None, hst=(h.t, h.dt, nlim if nlim >= 0 else None))
                        for _ in range(target.write_history_rows(h, outputs)):
                            h.t += h.dt
                            h.num += 1
                        if done > 0:
                            settled = h
            if done == 0:                         # ... and a dt that is not positive (or NaN) ends advance() with no step taken:
                target.step()                     # the single step goes on as the reference does (time = NaN ends the loop)
        outputs.data_output(target, 1)
    finally:
        if hasattr(outputs, "finish"):            # overlapped dumps: every file on disk when main returns
            outputs.finish()
