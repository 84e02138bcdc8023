"""Main loop of the reference (main.c:519-669) over a root Domain cut into x3 slabs, one slab
per process / GPU, with the reference's MPI calls replaced by torch.distributed (backend
"nccl" = RCCL over xGMI on MI355X; "gloo" in the CPU tests):

  * bvals_mhd's x3 Isend/Irecv pair (bvals_mhd.c:423-493)  -> batched isend/irecv of the packed
    4-plane halo (all i and j incl. ghosts so corners travel, bvals_mhd.c:170), both directions
    at once; periodic wrap = neighbour rank +-1 mod N exactly as the reference rewires lx/rx ids
  * MPI_Allreduce(MIN) of dt in new_dt (new_dt.c:177) and of dt_chem / dt_therm / dt_hydro, and
    SUM of the out-of-range cell count (ionrad_3d.c:275,399,554,672) -> all_reduce on small
    tensors; the four per-sub-cycle reductions collapse into two rounds
  * the domain is never cut along x1 (the ray direction), so the reference's rank pipeline of
    get_ph_rate_plane (ionradplane_3d.c:226-400) does not exist here.

All reductions are MIN/MAX of doubles or integer sums, hence bitwise independent of the
decomposition: an N-slab run reproduces the 1-slab run exactly for position-independent
problems (the reference has the same property).

The per-slab arithmetic is behind the small ``Engine`` interface; the product engine is
``HipEngine`` (the C-ABI library).  With one rank and no engine override the whole loop runs
inside the C library (aa_step) with no Python between kernels.
"""
from __future__ import annotations

import contextlib
import os
import warnings
from typing import List, Optional

import numpy as np

from . import config, dumps, restart
from .config import pencil, GridConfig, RunConfig, slab
from .history import HistoryWriter

MAXCELLCOUNT = 20   # ionrad.h:38


class HipEngine:
    """One slab on one MI355X, through include/athena_amd.h."""

    def __init__(self, grid: GridConfig, device: int = 0, strict: Optional[bool] = None, use_torch_stream: bool = True,
                 nslab: int = 1, initial: bool = True):
        """initial = False: no problem generator, the state comes from a restart dump (lib.setup_problem)"""
        import torch
        from . import lib
        self.torch = torch
        self.cfg = grid
        torch.cuda.set_device(device)
        # nslab > 1: the library cuts this Grid into x3 slabs itself (csrc/slabs.hip; one stream per slab, so the
        # caller's stream is not handed over)
        self.g = lib.setup_problem(grid, device, strict, nslab=nslab, initial=initial)
        if use_torch_stream and nslab == 1:
            # run the kernels on torch's current stream so that torch.distributed collectives and
            # torch.cuda.Event timing are ordered with them
            self.g.set_stream(torch.cuda.current_stream().cuda_stream)
        # Driver.step calls integrate -> userwork (pinned zones only) -> new_dt in that order: the update kernel may
        # leave new_dt's maxima behind (aa_cfl_in_update; AA_CFL_FUSED=0 keeps the separate sweep over the Grid)
        self.g.cfl_in_update(os.environ.get("AA_CFL_FUSED", "1") != "0")
        n = self.g.halo_doubles() if nslab == 1 else 0        # (slabs inside the library exchange their halos themselves)
        dev = torch.device("cuda", device)
        # the one-kernel radiation sub-cycle leaves this slab's reduction words in device memory; with several
        # ranks they are all-gathered on the stream (ONE collective per sub-cycle, no host round trip)
        self.ion_fused = bool(grid.run.ion) and self.g.ion_is_fused()
        self.words = torch.zeros(lib.ION_WORDS, dtype=torch.float64, device=dev)
        self.words_all = torch.zeros(lib.ION_WORDS * max(1, grid.nranks), dtype=torch.float64, device=dev)
        self.send = [torch.empty(n, dtype=torch.float64, device=dev) for _ in range(2)]
        self.recv = [torch.empty(n, dtype=torch.float64, device=dev) for _ in range(2)]
        n2 = self.g.halo_doubles_x2() if (nslab == 1 and grid.p2 > 1) else 0      # x2 x x3 pencils: the x2 halo as well
        self.send2 = [torch.empty(n2, dtype=torch.float64, device=dev) for _ in range(2)]
        self.recv2 = [torch.empty(n2, dtype=torch.float64, device=dev) for _ in range(2)]
        self.scalar_device = dev

    # slab arithmetic
    def bvals_local(self): self.g.bvals_mhd()
    def bvals_ionrad(self): self.g.bvals_ionrad()
    def new_dt_local(self) -> float: return self.g.new_dt_local()
    def integrate(self): self.g.integrate()
    def integrate_begin(self): self.g.integrate_begin()
    def userwork(self): self.g.apply_pinned_cells()
    def ion_begin(self): self.g.ion_begin()
    def ion_speculate(self, limit): self.g.ion_speculate(limit)
    def ion_rates(self): return self.g.ion_rates()
    def ion_update(self, dt): return self.g.ion_update(dt)
    def ion_pass(self, update, sweep): self.g.ion_pass(update, sweep, self.words.data_ptr())

    def ion_pick(self, dist, first, limit):
        """the step of the sub-cycle from the words of all slabs (ionrad_3d.c:399,:554,:275,:672 in one round)"""
        if dist is None:
            self.g.ion_pick(self.words.data_ptr(), 1, first, limit)
            return
        if dist.get_backend() == "gloo":                     # rehearsal on one GPU: gloo moves host tensors
            w = self.words.cpu(); wa = self.words_all.cpu()
            dist.all_gather_into_tensor(wa, w)
            self.words_all.copy_(wa)
        else:
            dist.all_gather_into_tensor(self.words_all, self.words)
        self.g.ion_pick(self.words_all.data_ptr(), self.cfg.nranks, first, limit)

    def ion_fetch(self): return self.g.ion_fetch()
    def ion_finish(self): self.g.ion_finish()

    def ion_radtransfer_gather(self, dist) -> int:
        """the whole sub-cycle loop inside the library (aa_ion_radtransfer_3d_gather): the only thing left to this side is the
        all-gather of the slabs' words, once per pass -- ONE crossing per sub-cycle, as a one-rank run has none"""
        if dist.get_backend() == "gloo":                     # rehearsal on one GPU: gloo moves host tensors
            def gather():
                w = self.words.cpu(); wa = self.words_all.cpu()
                dist.all_gather_into_tensor(wa, w)
                self.words_all.copy_(wa)
        else:
            def gather():
                dist.all_gather_into_tensor(self.words_all, self.words)
        return self.g.ion_radtransfer_3d_gather(self.words.data_ptr(), self.words_all.data_ptr(), self.cfg.nranks, gather)

    def host_syncs(self, reset=False): return self.g.host_syncs(reset)
    def set_mesh_state(self, time, dt, nstep): self.g.set_mesh_state(time, dt, nstep)
    def has_radiation(self) -> bool: return self.g.has_radplane()      # main.c:546, as aa_step: the ion step runs iff nradplane > 0
    def step_local(self) -> int: return self.g.step()

    def can_batch(self) -> bool:
        """a 1-D Grid aa_run_1d takes (it fits the resident kernel and has no pinned zones): run_local takes whole stretches of the
        main loop in one launch; or a 2-D Grid aa_run_2d takes (no pinned zones, not a level of a Mesh) unless AA_2D_BATCH=0:
        run_local queues AA_2D_BATCH steps per read-back; or a 3-D hydro Grid aa_run_3d queues (the default CTU chain, no pinned
        zones, no slabs, not a level of a Mesh) unless AA_3D_BATCH=0; every other Grid steps one at a time"""
        if self.g.ndim == 2:
            return self.g.run_2d_batch() != 0 and self.g.can_run_2d()
        if self.g.ndim == 3 and hasattr(self.g, "can_run_3d"):      # (a Grid object without the 3-D call steps one at a time, as before it existed)
            return self.g.can_run_3d() and self.g.run_3d_batch() != 0
        return self.g.can_run_until()

    def hst_route(self):
        """None where a history schedule rides on run_local (lib.Grid.run_hst_arm); else (kind, reason) for the one warning"""
        if self.g.ndim == 1:
            return ("1-D", "a 1-D Grid keeps its whole loop in one launch (aa_run_1d sums in another order)")
        if self.g.composite:
            return ("slabs", "a Grid cut into slabs inside the library steps one at a time")
        return None

    def hst_rows(self):
        """(rows[n][11], t_next) of the run_local call that had a schedule armed"""
        return self.g.run_hst_rows()

    def run_local(self, t_stop: float, tlim: float, nstep_stop, hst=None) -> int:
        """hst = (t_next, dt_out, nlim): a history schedule for this call alone (hst_route() is None)"""
        if hst is not None:
            self.g.run_hst_arm(*hst)
        if self.g.ndim == 2:
            return self.g.run_2d(t_stop, tlim, nstep_stop)
        if self.g.ndim == 3:
            return self.g.run_3d(t_stop, tlim, nstep_stop)
        return self.g.run_until(t_stop, tlim, nstep_stop)
    def start_local(self): self.g.start()
    def resume_local(self): self.g.resume()
    def write_rst_payload(self, f): self.g.write_rst_payload(f)
    def read_rst_payload(self, f): self.g.read_rst_payload(f)
    def read_rst_boxes(self, sources, rootNx, lo, n): self.g.read_rst_boxes(sources, rootNx, lo, n)
    def write_rst_box_payload(self, f, lo, n): self.g.write_rst_box_payload(f, lo, n)
    def mesh_state(self): return self.g.mesh_state()

    # halo
    def pack_x3(self, side: int):
        self.g.pack_x3(side, self.send[side].data_ptr()); return self.send[side]

    def recv_buffer(self, side: int): return self.recv[side]
    def unpack_x3(self, side: int): self.g.unpack_x3(side, self.recv[side].data_ptr())

    def pack_x2(self, side: int):
        self.g.pack_x2(side, self.send2[side].data_ptr()); return self.send2[side]

    def recv_buffer_x2(self, side: int): return self.recv2[side]
    def unpack_x2(self, side: int): self.g.unpack_x2(side, self.recv2[side].data_ptr())
    def bvals_side(self, dir: int, side: int): self.g.bvals_mhd_side(dir, side)
    def sync(self): self.g.sync()
    def download(self) -> np.ndarray: return self.g.download()
    def download_edgeflux(self) -> np.ndarray: return self.g.download_edgeflux()
    def history(self) -> np.ndarray: return self.g.history()

    def write_dump(self, path: str, fmt, prim: bool, time: float, dt: float):
        """dump_vtk / dump_binary of this slab: the payload comes from the device in file order (csrc/dump.hip)"""
        self.g.write_dump(path, fmt, prim, time=time, dt=dt)

    def outdata(self, expr, reduce, lo, hi): return self.g.outdata(expr, reduce, lo, hi)
    def outdata_gray(self, expr, reduce, lo, hi, dmin, dmax): return self.g.outdata_gray(expr, reduce, lo, hi, dmin, dmax)

    def dump_source(self):
        """what takes the snapshots of an overlapped dump (outputs.OutputSet.overlapped_dump / overlapped_restart): this slab's Grid"""
        return self.g

    def fofc_counts(self): return self.g.fofc_counts()
    def close(self): self.g.close()


def _active(U: np.ndarray) -> np.ndarray:
    """the active zones of a host block [N3][N2][N1][nvar]; a direction with one zone has no ghost zones (a 2-D Grid: N3 = 1, a
    1-D Grid: N2 = N3 = 1)"""
    ng = config.NGHOST
    k = slice(ng, -ng) if U.shape[0] > 1 else slice(None)
    j = slice(ng, -ng) if U.shape[1] > 1 else slice(None)
    return U[k, j, ng:-ng]


def _fires(out, level: int, domain: int = 0) -> bool:
    """whether an <outputN> block asks for this Domain (level / domain = -1: all of them; output.c:509-560)"""
    return out.level in (-1, level) and out.domain in (-1, domain)


def pick_step(dt_chem, dt_therm, dt_done, limit):
    """ionrad_3d.c:941-962: MIN(dt_therm, dt_chem), cut back so that dt_done + dt does not pass `limit` (root: the hydro step;
    refined level: tcoarse) -> (dt, whether it was cut back: hydro_done / coarsetime_done)"""
    dt = dt_therm if dt_therm < dt_chem else dt_chem
    if dt_done + dt > limit:
        return limit - dt_done, True
    return dt, False


def subcycles(one, fine):
    """The radiation sub-cycle loop ionrad_3d.c:919-1012, however a sub-cycle is issued: one(dt_done) performs the sub-cycle that
    starts at dt_done (with its collectives) and returns (the step it applied, whether that step was cut back to the limit, cells
    out of range, dt_hydro).  The root ends on check_range, on the covered step, on dt_hydro -- in this order; a refined level
    only when tcoarse is covered.  Nothing caps the count (maxiter: close_root).  -> (niter, dt_done, whether the level's dt
    becomes dt_done).  csrc/ion_subcycle.h is the same loop for the library; tests/test_ion_subcycles.py scripts both."""
    dt_done, niter = 0.0, 0
    while True:
        dt, hit, cellcount, dt_hydro = one(dt_done)
        dt_done += dt                                   # :966-967
        niter += 1
        if fine:
            if hit:                                     # :1008-1012
                return niter, dt_done, True
        elif cellcount > MAXCELLCOUNT:                  # :982-986 check_range
            return niter, dt_done, True
        elif hit:                                       # :989-992
            return niter, dt_done, False
        elif dt_hydro < dt_done:                        # :997-1002
            return niter, dt_done, True


def close_root(niter, maxiter, dt, dt_done):
    """The root level behind its loop, ionrad_3d.c:1017-1029 and :1044 -> (the root's dt, tcoarse)"""
    if niter == maxiter:
        dt = dt_done
    if dt < 0:
        raise RuntimeError(f"[ion_radtransfer_3d]: dt = {dt}")
    return dt, dt_done


def fold_levels(v, dx, ndir=3):
    """new_dt.c:33 and :156-161 over the levels of a Mesh: v holds max(|v_d| + a) per level and direction (3 per level), dx the zone
    sizes per level.  The maxima are carried from level to level (max_v1..3 are zeroed once, in front of the loop over Grids), and
    every level folds (carried maximum)/dx_d into max_dti over its first ndir directions -> max_dti.  One level: new_dt of a Grid.
    csrc/time_step.h is the same rule for the library, the kernels and the shim; tests/test_time_step.py scripts both."""
    cum, max_dti = [0.0, 0.0, 0.0], 0.0
    for l in range(len(dx)):
        for d in range(ndir):
            cum[d] = cum[d] if cum[d] > v[3 * l + d] else v[3 * l + d]
        for d in range(ndir):
            q = cum[d] / dx[l][d]
            max_dti = max_dti if max_dti > q else q
    return max_dti


def pick_dt(nstep, dt, dt_cfl, time, tlim):
    """new_dt.c:167-185: the CFL step, at most twice the last one (not on step 0) -- MIN(a,b) = (a < b) ? a : b (defs.h.in:146), so a
    NaN dt_cfl gives NaN, where min() would return 2*dt -- then cut back so that the loop ends at tlim exactly"""
    if nstep != 0:
        dt_cfl = 2.0 * dt if 2.0 * dt < dt_cfl else dt_cfl
    if time < tlim and (tlim - time) < dt_cfl:
        dt_cfl = tlim - time
    return dt_cfl


def _fetched(fetch):
    """the read-back of a one-kernel sub-cycle (aa_ion_fetch) as subcycles() takes it"""
    dt, hit, _dt_chem, _dt_therm, cellcount, dt_hydro, neg = fetch
    if neg:
        raise RuntimeError("[compute_chem_rates]: negative dt_chem")           # ionrad_3d.c:389-391
    return dt, hit, cellcount, dt_hydro


class _Runner:
    """What Driver, MeshRun and MeshDriver share: the scalar collectives, continuing from a restart dump, and the output side that
    outputs.OutputSet drives.  A runner has `run`, `time`, `dt`, `nstep`, `restarted`, `par` and the HistoryWriters `_hst`."""

    def _init_collectives(self, rank: int, nranks: int):
        # AA_FORCE_DISTRIBUTED=1 runs the Python-orchestrated loop (with its collectives) even on one
        # rank: used to rehearse the N>1 code path on a single GPU
        self.distributed = nranks > 1 or bool(os.environ.get("AA_FORCE_DISTRIBUTED"))
        self._py_syncs = 0        # host round trips of collectives issued from here (bench: host_syncs_per_step)
        if self.distributed:
            import torch
            import torch.distributed as dist
            self.torch, self.dist = torch, dist
            assert dist.is_initialized() and dist.get_world_size() == nranks and dist.get_rank() == rank
            self._sdev = getattr(self.eng, "scalar_device", torch.device("cpu"))

    def _allreduce(self, vals, op):
        if not self.distributed:
            return list(vals)
        t = self.torch.tensor(list(vals), dtype=self.torch.float64, device=self._sdev)
        self.dist.all_reduce(t, op=op)
        self._py_syncs += 1
        return t.tolist()

    # ---- continuing a run (main.c -r) ------------------------------------------------------------------
    @staticmethod
    def _resume_head(path, overrides, problem, integrator, order, order_2d: int = 2):
        """(head of rank 0's file, its parameter table with the overrides on top, the RunConfig built from that)"""
        head0 = restart.read_head(path)
        par = head0["par"].cmdline(overrides)
        run = config.from_par(par, problem)
        if integrator not in ("ctu", "vl", "ctu-noh"):
            raise config.ParError(f"[integrate_init]: unknown integrator {integrator}")
        run.integrator, run.order = integrator, order
        run.order_2d = int(order_2d)      # (a build option of the reference, --with-order, like the integrator: not in the file)
        config.check_2d(run)
        config.check_1d(run)
        return head0, par, run

    def _read_rank_file(self, head0, nxs, per_level: bool):
        """This rank's file (restart.rank_path) into the engine: the sections of the Grids of `nxs` active zones, root first, by
        read_rst_payload or, for an engine that keeps host blocks, load_state; per_level: both take the level first.
        -> the file's head"""
        run, eng = self.run, self.eng
        head = head0 if self.rank == 0 else restart.read_head(restart.rank_path(head0["path"], self.rank))
        head["levels"] = restart.index_sections(head, nxs, run.nscal, run.ion)
        lev = (lambda l: (l,)) if per_level else (lambda l: ())
        if hasattr(eng, "read_rst_payload"):
            with open(head["path"], "rb") as f:
                f.seek(head["offset"])
                for l in range(len(nxs)):
                    eng.read_rst_payload(*lev(l), f)
        elif hasattr(eng, "load_state"):
            for l, nx in enumerate(nxs):
                eng.load_state(*lev(l), *restart.read_state(head, l, nx, run.nscal))
        else:
            raise RuntimeError("[restart_grids]: this engine takes no state (read_rst_payload or load_state)")
        return head

    def _resumed(self, head, par):
        """time, dt and nstep of the file into the runner and its engine (_set_state); start() is then the restarted run's"""
        self._set_state(head["time"], head["dt"], head["nstep"])
        self.restarted, self.par = True, par

    @staticmethod
    def _mesh_sources(head0, par, run):
        """regrid = True of MeshRun / MeshDriver.from_restart: (the Domains of the file's table -- config.levels --, per Domain the
        Grids of the run that wrote the files with the file each lies in -- restart.scan_mesh_sources)"""
        if run.ndim == 2:
            raise restart.RestartError("[restart_grids]: regrid is not built for a 2-D mesh (Nx3 = 1): its files are read on the "
                                       "cuts that wrote them")
        doms = config.levels(par, run)
        return doms, restart.scan_mesh_sources(head0["path"], doms, run.nscal, run.ion, head0)

    # ---- outputs (output.c:498-569; outputs.OutputSet drives these) -----------------------------
    @contextlib.contextmanager
    def _rst_file(self, out, outputs, rel=None, table=None):
        """dump_restart's file, open between header and trailer: the time and the step count go into the parameter table first
        (restart.c:522-523), the table as it then stands -- or table(it) -- is the file's parameter dump.  rel: the path
        under the rank's directory, by default ath_fname's."""
        par = outputs.par
        par.blocks.setdefault("time", {})["time"] = "%e" % self.time
        par.blocks["time"]["nstep"] = "%d" % self.nstep
        rel = rel or dumps.fname(outputs.basename, 0, 0, out.num, "rst")
        with open(outputs.path(rel), "wb") as f:
            restart.write_header(f, restart.par_dump(table(par) if table else par), self.nstep, self.time, self.dt)
            yield f
            restart.write_trailer(f)

    def _write_restart_mesh_split(self, out, outputs, Nxs, box_payload):
        """OutputSet(rst_mesh_ngrid=...): one file per rank of a run of the reference whose Domains (of `Nxs` zones, level by level)
        are cut by those NGrid_x* -- ``id<r>/<base>[-id<r>].NNNN.rst`` holding, in Domain order, the sections of the Grids
        restart.mesh_grid_boxes deals to rank r, under a table with NGrid_x* of every <domainN> set, no AutoWithNProc, and its
        own problem_id.  box_payload(n, f, lo, nx) writes the sections of the box [lo, lo + nx) of Domain n."""
        ngrids = outputs.rst_mesh_ngrid
        if len(ngrids) != len(Nxs):
            raise ValueError(f"[dump_restart]: rst_mesh_ngrid names {len(ngrids)} Domains, the mesh has {len(Nxs)}")
        table = restart.mesh_grid_boxes(list(zip(Nxs, ngrids)), outputs.rst_mesh_nproc)
        for r in range(outputs.rst_mesh_nproc):
            base = outputs.basename + ("-id%d" % r if r else "")
            rel = os.path.join("id%d" % r, dumps.fname(base, 0, 0, out.num, "rst"))
            with self._rst_file(out, outputs, rel, lambda par: restart.regrid_mesh_par(par, ngrids, r, outputs.basename)) as f:
                for n, boxes in enumerate(table):
                    for rank, lo, nx in boxes:
                        if rank == r:
                            box_payload(n, f, lo, nx)

    def _host_state(self, *level):
        """(U of the active zones, EdgeFlux or None) from the host block of an engine that has no write_rst_payload: what
        restart.write_grid_sections takes.  level: none for Driver's engine, (l,) for MeshDriver's."""
        U = _active(self.eng.download(*level))[..., :5 + self.run.nscal]
        ef = None
        if self.run.ion:
            edgeflux = getattr(self.eng, "edgeflux" if level else "download_edgeflux", None)
            if edgeflux is None:
                raise RuntimeError("[dump_restart]: this engine cannot hand out GridS.EdgeFlux")
            ef = edgeflux(*level)
        return U, ef

    def _domain_volume(self, Nx, level: int) -> float:
        """of a Domain of Nx zones of a refined mesh (Driver has its own: the root Domain's, from its edges)"""
        vol = 1.0
        for a in range(3):
            if a == 0 or Nx[a] > 1:               # dump_history.c:316-321: a direction with one zone (x3 of a 2-D Domain) does not count
                vol *= Nx[a] * (self.run.dx[a] / float(1 << level))
        return vol

    def _history_row(self, key, rundir, level, domain, out, outputs, sums, vol, time=None, dt=None):
        """One row of the .hst file of a Domain of volume `vol` (dump_history.c:271-279, :328-361): `sums` are its volume
        integrals, already added over its Grids; the writer is kept under `key` for the rows to come.  time, dt: of the row
        where it was made behind an earlier step than the last (a queued run's rows, write_history_rows); default: of now."""
        w = self._hst.get(key)
        if w is None:
            w = self._hst[key] = HistoryWriter(rundir, outputs.basename, level, domain, out.dat_fmt, num=out.num)
        w.dump(self.time if time is None else time, self.dt if dt is None else dt, sums, vol, self.run.nscal)
        rel = os.path.relpath(w.path, outputs.dir)
        if rel not in outputs.written:
            outputs.written.append(rel)

    def data_output(self, outputs, flag: int):
        """data_output(&Mesh, flag) of main.c: see outputs.OutputSet.data_output"""
        outputs.data_output(self, flag)

    def single_route(self, outputs):
        """None where this runner writes the single-variable blocks of OutputSet.from_par(single=True), else the reason it
        refuses the keyword (asked once, before the first output)"""
        return f"{type(self).__name__} writes no single-variable outputs"

    def main(self, outputs):
        """main.c:501-743: start, forced output (not after a restart), the loop up to <time>tlim / nlim with data_output(0) at
        the top of every pass, forced output.  Every rank of a multi-rank run calls it with its own
        OutputSet.from_par(par, time, rundir, rank, nranks) and writes its own Grids."""
        from . import outputs as _outputs
        _outputs.run(self, outputs, self.run.tlim, self.run.nlim)


_ION_BATCH_WARNED = False      # Driver(ion_batch=...) with several ranks warns once per process


class Driver(_Runner):
    """main() of the reference for one process of an N-process run."""

    def __init__(self, run: RunConfig, engine_factory=None, rank: int = 0, nranks: int = 1, device: int = 0,
                 strict: Optional[bool] = None, p2: int = 1, initial: bool = True, ion_batch: Optional[int] = None):
        """p2 > 1: an NGrid_x2 x NGrid_x3 = p2 x (nranks / p2) pencil decomposition (init_mesh.c:526-620) instead of x3 slabs;
        initial = False: the product engine skips the problem generator (from_restart loads the state);
        ion_batch = K (1 .. 256; None: nothing changes): on one rank with an engine on a device the ion step is the library's loop
        (lib.Grid.ion_radtransfer_3d) with K sub-cycles queued per host visit (lib.Grid.set_ion_batch) instead of the loop written
        here; same bits.  With several ranks the keyword warns once and the step stays what it was."""
        self.run = run
        self.rank, self.nranks = rank, nranks
        if p2 < 1 or nranks % p2:
            raise ValueError(f"{nranks} ranks cannot be dealt {p2} along x2")
        config.check_fofc(run, nranks)      # (ParError: first-order flux correction is a single-Grid feature)
        config.check_2d(run, nranks)      # (ParError: a 2-D run is one Grid on one rank)
        config.check_1d(run, nranks)      # (... and so is a 1-D run)
        self.fofc_trace: List[Tuple[int, int, int]] = []    # run.fofc: (zones with d < 0, with P < 0, fluxes replaced) of every step
        self.grid = pencil(run, rank, p2, nranks // p2)
        self.eng = engine_factory(self.grid) if engine_factory else HipEngine(self.grid, device, strict, initial=initial)
        self.restarted = False    # from_restart: start() is the restarted run's, outputs.run skips the forced first output
        self.par = None           # the parameter table this Driver was built from (from_restart)
        self.time, self.dt, self.nstep = 0.0, 0.0, 0
        self.niter_trace: List[int] = []
        self._hst = {}            # HistoryWriter per <outputN> block with out_fmt = hst
        self._halo = {}           # messages in flight per axis (2: x2, 3: x3): post .. finish
        self._init_collectives(rank, nranks)
        self.ion_batch = None
        if ion_batch is not None:
            global _ION_BATCH_WARNED
            if nranks > 1:
                if not _ION_BATCH_WARNED:
                    warnings.warn("Driver(ion_batch=...): several ranks reduce every sub-cycle over the ranks; the keyword is ignored")
                    _ION_BATCH_WARNED = True
            elif hasattr(getattr(self.eng, "g", None), "set_ion_batch"):
                self.eng.g.set_ion_batch(ion_batch)
                self.ion_batch = int(ion_batch)

    @classmethod
    def from_restart(cls, path: str, overrides=(), problem: Optional[str] = None, integrator: str = "ctu", order: int = 2,
                     engine_factory=None, rank: int = 0, nranks: int = 1, device: int = 0, strict: Optional[bool] = None,
                     p2: int = 1, regrid: bool = False, fofc: bool = False, order_2d: int = 2) -> "Driver":
        """``athena -r path [block/key=value ...]`` (main.c:168-173, :216-288; restart_grids, restart.c:52-456).  `path` is
        rank 0's file: every rank takes the parameter table from it, with the overrides on top (an unknown key is an error;
        time/nlim and time/tlim extend a run), and reads its own Grid from restart.rank_path(path, rank).  The problem
        generator does not run; the hooks are registered as by problem_read_restart.  The Driver keeps the table as `.par`:
        OutputSet.from_par(d.par, d.time, rundir, rank, nranks) continues the numbering of every <outputN> block.

        regrid = True resumes on THIS Driver's decomposition (rank, nranks, p2) whatever cuts wrote the files -- the file's own
        ``<domain1> NGrid_x1/2/3``, x1 cuts included: every rank reads, from every source file that meets its Grid, the part
        that does (restart.scan_sources, restart.box_pieces); time, dt and nstep are rank 0's file's.  `.par` then names the new
        cuts (NGrid_x1 = 1, NGrid_x2 = p2, NGrid_x3 = nranks / p2, no AutoWithNProc), so that a later dump describes itself.
        Single-level meshes only.

        order_2d = 3 resumes a 2-D run (Nx3 = 1) at third order (config.RunConfig.order_2d): the reference's order is a build option
        and is not in the file."""
        head0, par, run = cls._resume_head(path, overrides, problem, integrator, order, order_2d)
        if regrid and run.ndim == 1:
            raise restart.RestartError("[restart_grids]: regrid is not built for a 1-D Grid (Nx2 = Nx3 = 1): it is one Grid on one rank")
        run.fofc = bool(fofc)      # (a build option of the reference like the integrator: not in the file; it carries no state between steps)
        sources = restart.scan_sources(path, run.rootNx, run.nscal, run.ion, head0) if regrid else None
        d = cls(run, engine_factory, rank, nranks, device, strict, p2, initial=False)
        if not regrid:
            d._resumed(d._read_rank_file(head0, [d.grid.Nx], per_level=False), par)
            return d
        if hasattr(d.eng, "read_rst_boxes"):
            d.eng.read_rst_boxes(sources, run.rootNx, d.grid.disp, d.grid.Nx)
        elif hasattr(d.eng, "load_state"):
            d.eng.load_state(*restart.read_state_boxes(sources, run.rootNx, d.grid.disp, d.grid.Nx, run.nscal))
        else:
            raise RuntimeError("[restart_grids]: this engine takes no state (read_rst_boxes or load_state)")
        d._resumed(head0, restart.regrid_par(par, (1, p2, nranks // p2)))
        return d

    def _set_state(self, time, dt, nstep):
        self.time, self.dt, self.nstep = time, dt, nstep
        self.eng.set_mesh_state(time, dt, nstep)

    # ---- collectives ------------------------------------------------------------------
    def host_sync_count(self, reset: bool = False) -> int:
        """Times the host waited for the device to hand back scalars (library read-backs + collectives' .tolist())."""
        n = self._py_syncs + (self.eng.host_syncs(reset) if hasattr(self.eng, "host_syncs") else 0)
        if reset:
            self._py_syncs = 0
        return n

    def _min(self, *vals): return self._allreduce(vals, self.dist.ReduceOp.MIN if self.distributed else None)

    def history(self) -> np.ndarray:
        """dump_history.c:157-260: this slab's volume integrals, added over the slabs of the Domain
        (the reference's MPI_Reduce(SUM) :257; here an all-reduce so every rank may write)."""
        s = self.eng.history()
        if self.distributed:
            s = np.array(self._allreduce(s, self.dist.ReduceOp.SUM))
        return s

    def dump_history(self, writer):
        """One row of the .hst file (history.HistoryWriter); call it where main.c calls data_output."""
        s = self.history()
        if self.rank == 0:
            writer.dump(self.time, self.dt, s, self._volume(), self.run.nscal)

    def _volume(self) -> float:
        """of the root Domain, from its edges: not always the double that Nx * dx gives (_Runner._domain_volume)"""
        vol = 1.0
        for d in range(3):
            if d == 0 or self.run.rootNx[d] > 1:      # dump_history.c:316-321: a direction with one zone does not count
                vol *= self.run.xmax[d] - self.run.xmin[d]
        return vol

    # ---- outputs (output.c:498-569; outputs.OutputSet drives these) -----------------------------
    def write_dump(self, out, outputs):
        """dump_vtk / dump_binary of this rank's Grid (level 0, domain 0) for one <outputN> block."""
        if not _fires(out, 0):
            return
        g, r = self.grid, self.run
        rel = dumps.fname(outputs.basename, 0, 0, out.num, out.out_fmt)
        if getattr(outputs, "overlap", False):    # snapshot now, copy and file write beside the next steps -- where the engine has a device
            src = self.eng.dump_source() if hasattr(self.eng, "dump_source") else None
            if outputs.overlapped_dump(src, rel, out.out_fmt, out.prim, time=self.time, dt=self.dt):
                return
        path = outputs.path(rel)
        if hasattr(self.eng, "write_dump"):
            self.eng.write_dump(path, out.out_fmt, out.prim, self.time, self.dt)
        else:                                     # an engine without a device: the same payload from its host block
            U = _active(self.eng.download())
            dumps.write_dump_from_block(path, out.out_fmt, U, prim=out.prim, gamma=r.gamma, nscal=r.nscal, nx=g.Nx,
                                        minx=g.MinX, dx=r.dx, time=self.time, dt=self.dt)

    def single_route(self, outputs):
        if self.nranks > 1:
            return "a Driver on several ranks holds a part of every slice; single-variable outputs take one rank"
        if self.run.ndim == 1:
            return "a 1-D Grid (Nx2 = Nx3 = 1) is not built"
        if getattr(getattr(self.eng, "g", None), "composite", False):
            return "a Grid cut into slabs inside the library makes no single-variable output (one Grid on one device does)"
        if any(o.single and o.out == "flux" for o in outputs.outs) and self.run.problem != "ioniz_sphere":
            return f"out = flux: problem \"{self.run.problem}\" defines no such expression (ioniz_sphere does)"
        return None

    def write_single(self, out, outputs):
        """output_vtk / output_tab / output_pgm of this Grid for one single-variable <outputN> block (output.c OutData1/2/3): the
        payload, its minimum and maximum and the gray bytes from the device where the engine has one (lib.Grid.outdata), else the
        same arithmetic in numpy over the engine's host block.  A slice that misses the Grid writes no file."""
        if not _fires(out, 0):
            return
        from . import outputs as _o
        g, r = self.grid, self.run
        rng = _o.single_ranges(out, g.Nx, g.MinX, r.dx)
        if rng is None:
            return
        reduce, lo, hi = rng
        shape = _o.payload_shape(reduce, g.Nx)
        on_device = hasattr(self.eng, "outdata")
        if on_device:
            data, dmin, dmax = self.eng.outdata(out.out, reduce, lo, hi)
        else:
            U = self.eng.download()
            first = [config.NGHOST if n > 1 else 0 for n in g.Nx]
            V = dumps.expr_from_block(U, out.out, r.gamma, self.eng.download_edgeflux() if out.out == "flux" else None)
            if out.out == "flux":
                first = [0, 0, 0]
            full = [(lo[a], hi[a]) if reduce[a] else (0, g.Nx[a] - 1) for a in range(3)]
            data = dumps.outdata_from_values(V, first, reduce, [f[0] for f in full], [f[1] for f in full])
            dmin, dmax = dumps.minmax(data)
        data = np.asarray(data).reshape(shape)
        fmt = out.out_fmt
        if fmt == "tab" and len(shape) >= 2 and out.num == 0:       # output_tab.c:198-204, :273-279
            out.gmin, out.gmax = dmin, dmax
        else:                                                       # MIN / MAX of the writers (output_vtk.c:112-113, output_pgm.c:87-88)
            out.gmin = dmin if dmin < out.gmin else out.gmin
            out.gmax = dmax if dmax > out.gmax else out.gmax
        if fmt == "vtk":
            b = dumps.single_vtk_bytes(data, out.id, nx=g.Nx, minx=g.MinX, dx=r.dx, raw_reduce=out.raw_reduce, time=self.time)
        elif fmt == "tab":
            b = dumps.single_tab_bytes(data, out.dat_fmt)
        else:
            if out.sdmin:
                dmin = out.dmin
            if out.sdmax:
                dmax = out.dmax
            gray = self.eng.outdata_gray(out.out, reduce, lo, hi, dmin, dmax) if on_device else dumps.pgm_gray(data, dmin, dmax)
            b = dumps.single_pgm_bytes(gray, shape[1], shape[0])
        with open(outputs.path(dumps.fname_id(outputs.basename, 0, 0, out.num, out.id, fmt)), "wb") as f:
            f.write(b)

    def write_history(self, out, outputs):
        if not _fires(out, 0):
            return
        s = self.history()                        # (every rank takes part in the sum; rank 0 writes)
        if self.rank == 0:
            self._history_row(out.n, outputs.dir, 0, 0, out, outputs, s, self._volume())

    def write_restart(self, out, outputs):
        """dump_restart (restart.c:463-983): this rank's Grid under the parameter table as it stands now."""
        if getattr(outputs, "rst_ngrid", None):
            if getattr(outputs, "overlap_rst", False):
                outputs.overlap_fallback("rst_ngrid", "restart dumps cut for other Grids (rst_ngrid) take the boxes of "
                                         "aa_rst_section_get_box", "overlap_rst")
            return self._write_restart_split(out, outputs)
        if getattr(outputs, "overlap_rst", False):    # snapshot now, copy and file write beside the next steps -- where the engine has a device
            src = self.eng.dump_source() if hasattr(self.eng, "dump_source") else None
            rel = dumps.fname(outputs.basename, 0, 0, out.num, "rst")
            if outputs.overlapped_restart([src], rel, self.nstep, self.time, self.dt):
                return
        with self._rst_file(out, outputs) as f:
            if hasattr(self.eng, "write_rst_payload"):    # the sections come from the device in file order (csrc/restart.hip)
                self.eng.write_rst_payload(f)
            else:
                restart.write_grid_sections(f, *self._host_state())

    def _write_restart_split(self, out, outputs):
        """OutputSet(rst_ngrid=...): one file per Grid of restart.grid_boxes, ``id<r>/<base>[-id<r>].NNNN.rst`` as the ranks of a
        run on those cuts would leave them -- each under a table with NGrid_x* set to the target and its own problem_id, each
        with the box of every section (EDGEFLUX with its n + 1 faces)."""
        if self.nranks > 1:
            raise ValueError("[dump_restart]: rst_ngrid takes a one-rank run")
        U = ef = None
        if not hasattr(self.eng, "write_rst_box_payload"):
            U, ef = self._host_state()
        for r, lo, n in restart.grid_boxes(self.run.rootNx, outputs.rst_ngrid):
            base = outputs.basename + ("-id%d" % r if r else "")
            rel = os.path.join("id%d" % r, dumps.fname(base, 0, 0, out.num, "rst"))
            with self._rst_file(out, outputs, rel,
                                lambda par: restart.regrid_par(par, outputs.rst_ngrid, r, outputs.basename)) as f:
                if U is None:
                    self.eng.write_rst_box_payload(f, lo, n)
                else:
                    k, j, i = (slice(lo[d], lo[d] + n[d]) for d in (2, 1, 0))
                    k1, j1, i1 = (slice(lo[d], lo[d] + n[d] + 1) for d in (2, 1, 0))
                    restart.write_grid_sections(f, U[k, j, i], None if ef is None else ef[k1, j1, i1])

    def exchange_x3(self):
        """bvals_mhd.c:423-493 for the x3 direction."""
        self.post_x3()
        self.finish_x3()

    def post_x3(self): self._post(3)
    def finish_x3(self): self._finish(3)

    def _post(self, axis: int):
        """The sends and receives of bvals_mhd.c:296-493 along one direction (pack_i* / pack_o*, MPI_Isend / MPI_Irecv)
        without the wait; axis 2 = x2 (pencils only), 3 = x3.  With RCCL the messages travel on the communicator's stream
        from here on; _finish() makes the kernel stream wait for them and unpacks.  What is queued in between must not
        touch the ghost zones of that direction or the buffers."""
        assert axis not in self._halo
        g, dist = self.grid, self.dist if self.distributed else None
        lo, hi = (g.lx2, g.rx2) if axis == 2 else (g.lx3, g.rx3)
        if not self.distributed or (lo < 0 and hi < 0):
            return
        e = self.eng
        pack = e.pack_x2 if axis == 2 else e.pack_x3
        recvb = e.recv_buffer_x2 if axis == 2 else e.recv_buffer
        host_stage = (dist.get_backend() == "gloo")   # gloo moves host tensors only

        def out(side):
            t = pack(side)
            return t.cpu() if (host_stage and t.is_cuda) else t

        rbuf = {}

        def inn(side):
            t = recvb(side)
            rbuf[side] = (self.torch.empty(t.shape, dtype=t.dtype) if (host_stage and t.is_cuda) else t)
            return rbuf[side]

        tag0 = 10 * axis
        if lo == hi and lo >= 0:
            # two Grids along this direction with periodic wrap: both messages go to the same peer; post them so that the
            # peer's inner planes (its first send) land in my OUTER ghosts (my first receive)
            ops = [dist.P2POp(dist.isend, out(0), lo, tag=tag0),
                   dist.P2POp(dist.isend, out(1), hi, tag=tag0 + 1),
                   dist.P2POp(dist.irecv, inn(1), hi, tag=tag0),
                   dist.P2POp(dist.irecv, inn(0), lo, tag=tag0 + 1)]
        else:
            ops = []
            # my inner planes fill the lower neighbour's outer ghosts, and vice versa
            if lo >= 0:
                ops.append(dist.P2POp(dist.isend, out(0), lo, tag=tag0))
                ops.append(dist.P2POp(dist.irecv, inn(0), lo, tag=tag0 + 1))
            if hi >= 0:
                ops.append(dist.P2POp(dist.isend, out(1), hi, tag=tag0 + 1))
                ops.append(dist.P2POp(dist.irecv, inn(1), hi, tag=tag0))
        self._halo[axis] = (dist.batch_isend_irecv(ops), rbuf)

    def _finish(self, axis: int):
        """MPI_Waitall + unpack_i* / unpack_o* of bvals_mhd.c:296-493."""
        if axis not in self._halo:
            return
        works, rbuf = self._halo.pop(axis)
        e = self.eng
        recvb = e.recv_buffer_x2 if axis == 2 else e.recv_buffer
        unpack = e.unpack_x2 if axis == 2 else e.unpack_x3
        for w in works:
            w.wait()
        for side in (0, 1):
            if side in rbuf:
                dst = recvb(side)
                if rbuf[side] is not dst:
                    dst.copy_(rbuf[side])
                unpack(side)

    # ---- the reference's call sites ---------------------------------------------------------
    def bvals_mhd(self, exchange: bool = True, wait: bool = True):
        if self.grid.p2 == 1:
            self.eng.bvals_local()      # x1, x2 and physical x3 faces
        else:
            # pencils: x1, then x2 (physical sides here, cut faces by messages), then x3 -- the order that carries the
            # corners (bvals_mhd.c:170); the x2 messages must have landed before x3 is packed
            for side in (0, 1):
                self.eng.bvals_side(0, side)
            for side in (0, 1):
                self.eng.bvals_side(1, side)
            if exchange:
                self._post(2)
                self._finish(2)
            for side in (0, 1):
                self.eng.bvals_side(2, side)
        if exchange:
            self.post_x3()
            if wait:
                self.finish_x3()

    def new_dt(self):               # new_dt.c:169-185
        dtc = self._min(self.eng.new_dt_local())[0] if self.distributed else self.eng.new_dt_local()
        self.dt = pick_dt(self.nstep, self.dt, dtc, self.time, self.run.tlim)
        self.eng.set_mesh_state(self.time, self.dt, self.nstep)

    def _ion_radtransfer_fused(self) -> int:
        """ionrad_3d.c:862-1047 with the one-kernel sub-cycle (include/athena_amd.h, aa_ion_pass): the loop is cut at
        the reduction that yields the step, so a sub-cycle is one pass, ONE all-gather of the slabs' words and one
        read-back; the sweep after a data-dependent stop is speculative and dropped by ion_finish."""
        e = self.eng
        dist = self.dist if self.distributed else None
        if dist is not None and hasattr(e, "ion_radtransfer_gather") and not os.environ.get("AA_DRIVER_PY_SUBCYCLES"):
            # the loop below inside the library, the all-gather as its callback (AA_DRIVER_PY_SUBCYCLES=1: the loop as written here)
            niter = e.ion_radtransfer_gather(dist)
            self.dt = e.mesh_state()[1]
            return niter
        limit = self.dt
        e.ion_begin()
        if hasattr(e, "ion_speculate"):
            e.ion_speculate(limit)          # the first pass may already apply the first update with the whole step
        e.ion_pass(False, True)
        e.ion_pick(dist, True, limit)

        def one(dt_done):
            e.ion_pass(True, True)          # the pass skips its sweep by itself once the step was cut back to the limit
            e.ion_pick(dist, False, limit)
            return _fetched(e.ion_fetch())  # the one read-back

        niter, dt_done, cut = subcycles(one, False)
        e.ion_finish()
        self.dt, _ = close_root(niter, self.run.maxiter, dt_done if cut else limit, dt_done)
        e.set_mesh_state(self.time, self.dt, self.nstep)
        return niter

    def ion_radtransfer(self) -> int:   # ionrad_3d.c:862-1047, root level
        e = self.eng
        if self.ion_batch is not None and not self.distributed:
            # the loop inside the library (aa_ion_radtransfer_3d: K sub-cycles per host visit where the Grid takes them); the
            # step it may have cut comes back as the gather branch's does
            niter = e.g.ion_radtransfer_3d()
            self.dt = e.mesh_state()[1]
            return niter
        if getattr(e, "ion_fused", False):
            return self._ion_radtransfer_fused()
        limit = self.dt
        e.ion_begin()

        def one(dt_done):
            dt_chem, dt_therm = e.ion_rates()
            if self.distributed:
                dt_chem, dt_therm = self._allreduce((dt_chem, dt_therm), self.dist.ReduceOp.MIN)
            dt, hit = pick_step(dt_chem, dt_therm, dt_done, limit)
            cellcount, dt_hydro = e.ion_update(dt)
            if self.distributed:
                # one round: SUM of the count and MIN of dt_hydro (as MAX of its negative)
                t = self.torch.tensor([float(cellcount), 0.0], dtype=self.torch.float64, device=self._sdev)
                h = self.torch.tensor([dt_hydro], dtype=self.torch.float64, device=self._sdev)
                w1 = self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM, async_op=True)
                w2 = self.dist.all_reduce(h, op=self.dist.ReduceOp.MIN, async_op=True)
                w1.wait(); w2.wait()
                cellcount, dt_hydro = int(t[0].item()), float(h[0].item())
            return dt, hit, cellcount, dt_hydro

        niter, dt_done, cut = subcycles(one, False)
        self.dt, _ = close_root(niter, self.run.maxiter, dt_done if cut else limit, dt_done)
        e.set_mesh_state(self.time, self.dt, self.nstep)
        return niter

    def _fofc_report(self):
        """The two lines integrate_3d_vl.c prints when the first-order flux correction did something (:898-901, :1281-1282)."""
        if not self.run.fofc or not hasattr(self.eng, "fofc_counts"):
            return
        negd, negP, nan = self.eng.fofc_counts()
        self.fofc_trace.append((negd, negP, nan))
        if nan != 0:
            print("[Step10] %i second-order fluxes replaced" % nan)
        if negd > 0 or negP > 0:
            print("[Step14]: %i cells had d<0; %i cells had P<0" % (negd, negP))

    # ---- main.c ---------------------------------------------------------------------------------
    def start(self):                # main.c:412-451
        if self.restarted:          # main.c:398-451 after restart_grids: the ghost zones, and NO new_dt -- the file's dt is the next step's
            if not self.distributed and hasattr(self.eng, "resume_local"):
                self.eng.set_mesh_state(self.time, self.dt, self.nstep)
                self.eng.resume_local()
                return
            self.eng.set_mesh_state(self.time, self.dt, self.nstep)
            self.bvals_mhd()
            self.eng.bvals_ionrad()
            return
        if not self.distributed and hasattr(self.eng, "start_local"):
            self.eng.start_local()
            self.time, self.dt, self.nstep = self.eng.mesh_state()
            return
        self.eng.set_mesh_state(self.time, self.dt, self.nstep)
        self.bvals_mhd()
        self.eng.bvals_ionrad()
        self.new_dt()

    def may_batch(self) -> bool:
        """whether advance() may take several steps in one call (outputs.run asks): one rank, and a 1-D Grid the resident kernel
        holds (aa_run_1d) or a 2-D / 3-D hydro Grid whose steps queue with the time step picked on the device (aa_run_2d, aa_run_3d)"""
        return not self.distributed and hasattr(self.eng, "can_batch") and self.eng.can_batch()

    def hst_route(self):
        """None where advance(..., hst=) makes the rows of a history block on the device (outputs.run with hst_queued asks); else
        (kind, reason): the block stays a stop time of the run"""
        if self.distributed:
            return ("ranks", "a Driver on several ranks adds the rows of its ranks on the host")
        if not hasattr(self.eng, "hst_route"):
            return ("engine", "this engine keeps no state on a device")
        return self.eng.hst_route()

    def write_history_rows(self, out, outputs) -> int:
        """the rows the last advance(..., hst=) made, each with its own time and dt, through the block's HistoryWriter -> their
        number (a row of a block that asks for another level or domain is made and counted, not written: _fires)"""
        rows, _ = self.eng.hst_rows()
        for r in rows:
            if _fires(out, 0):
                self._history_row(out.n, outputs.dir, 0, 0, out, outputs, r[2:], self._volume(), time=float(r[0]), dt=float(r[1]))
        return len(rows)

    def advance(self, t_stop: float, nstep_stop=None, hst=None) -> int:
        """Whole passes of the main loop until time >= t_stop or nstep == nstep_stop (None: no such limit), in one launch
        (aa_run_1d) or as queued steps with one read-back per batch (aa_run_2d, aa_run_3d); the same bits as that many step() calls.
        hst = (t_next, dt_out, nlim), where hst_route() is None: a history row behind every step that has one due
        (write_history_rows).  -> the steps taken"""
        far = self.nstep + (1 << 20)              # (aa_run_1d / aa_run_2d cover 2^20 steps per call at the most; the caller's loop goes on)
        stop = far if nstep_stop is None else min(int(nstep_stop), far)
        n = self.eng.run_local(t_stop, self.run.tlim, stop, hst) if hst is not None else self.eng.run_local(t_stop, self.run.tlim, stop)
        self.time, self.dt, self.nstep = self.eng.mesh_state()
        self.niter_trace.extend([0] * n)
        return n

    def step(self) -> int:          # main.c:519-669
        if not self.distributed and hasattr(self.eng, "step_local"):
            niter = self.eng.step_local()
            self._fofc_report()
            self.time, self.dt, self.nstep = self.eng.mesh_state()
            self.niter_trace.append(niter)
            return niter
        niter = 0
        if self.eng.has_radiation():
            niter = self.ion_radtransfer()
            # the x3 halo travels while the first-pass x1 / x2 sweeps of the planes ks..ke run (they read no
            # neighbour data: aa_integrate_begin); the rest of the integrator follows the unpack
            self.bvals_mhd(wait=False)
            if hasattr(self.eng, "integrate_begin"):
                self.eng.integrate_begin()
            self.finish_x3()
        self.eng.integrate()
        self._fofc_report()
        self.eng.userwork()
        self.nstep += 1
        self.time += self.dt
        self.new_dt()
        # main.c:635-644.  With radiation on, nothing reads the neighbour's planes before the bvals_mhd
        # that follows the next ion step (the ion kernels, new_dt and the dumps touch active zones only,
        # and that call re-sends every field anyway): the x3 halo of this call is left to it.
        self.bvals_mhd(exchange=not self.eng.has_radiation())
        self.niter_trace.append(niter)
        return niter


class MeshRun(_Runner):
    """main() of the reference built with STATIC_MESH_REFINEMENT for a lib.Mesh (all levels on one GPU; the loop itself is
    aa_mesh_step): what outputs.run / OutputSet.data_output need -- time, nstep, start, step and the three writers, which loop
    over the Domains like dump_vtk / dump_binary / dump_history / dump_restart do."""

    def __init__(self, mesh, run: RunConfig, nslab: int = 1, cuts=None, device: int = 0, strict: Optional[bool] = None,
                 ion_batch: Optional[int] = None):
        """ion_batch = K: lib.Mesh.set_ion_batch(K), the radiation sub-cycles every level queues per host visit (None: untouched).
        mesh: a lib.Mesh, or the levels (config.levels) to build one from -- with nslab > 1 / cuts every level cut at the
        same root x3 planes inside the library, one slab stack per GPU; the outputs go through the composite level handles
        as they are (hst per level, bin / vtk under lev<l>/, one .rst with all levels)."""
        config.check_1d(run, mesh=True)      # (ParError: a 1-D run has no Mesh)
        if isinstance(mesh, (list, tuple)):
            from . import lib
            mesh = lib.Mesh(list(mesh), device, strict, nslab=nslab, cuts=cuts)
        self.mesh, self.run = mesh, run
        if ion_batch is not None:
            mesh.set_ion_batch(ion_batch)
        self._hst = {}
        self.restarted = False
        self.par = None

    @classmethod
    def from_restart(cls, path: str, overrides=(), problem: Optional[str] = None, integrator: str = "ctu", order: int = 2,
                     device: int = 0, strict: Optional[bool] = None, nslab: int = 1, cuts=None, regrid: bool = False,
                     order_2d: int = 2) -> "MeshRun":
        """Driver.from_restart for a static-mesh-refinement deck: one file holds every Domain, root first (restart.c:531-770).
        nslab / cuts: resume on a Mesh cut into slabs inside the library, whatever wrote the file (lib.Mesh).

        regrid = True takes the files of an MPI run of the reference, `path` being rank 0's, whatever cuts wrote them: every
        <domainN> by its own NGrid_x1/2/3, x1 cuts included, the Grids dealt to the ranks as restart.mesh_grid_boxes states it,
        several Domains on a level included.  Every level reads, section by section, every source Grid's piece straight to the
        device (lib.Grid.read_rst_boxes); a level cut into slabs inside the library takes whole sections only, so one section
        of one level at a time is joined on the host (lib.Grid.read_rst_joined).  `.par` then names the decomposition this
        run is on (NGrid_x* = 1 in every <domainN>, no AutoWithNProc): its own dumps are read back without the keyword.

        order_2d = 3: every level of a 2-D Mesh resumes at third order (as Driver.from_restart)."""
        from . import lib
        head, par, run = cls._resume_head(path, overrides, problem, integrator, order, order_2d)
        if regrid:
            grids, sources = cls._mesh_sources(head, par, run)
            m = cls(lib.Mesh(grids, device, strict, initial=False, nslab=nslab, cuts=cuts), run)
            try:
                for g, cfg, src in zip(m.mesh.lev, grids, sources):
                    if m.mesh.cuts is not None:
                        g.read_rst_joined(src, cfg.Nx)
                    else:
                        g.read_rst_boxes(src, cfg.Nx, (0, 0, 0), cfg.Nx)
            except Exception:
                m.mesh.close()
                raise
            m._resumed(head, restart.regrid_mesh_par(par, [(1, 1, 1)] * len(grids)))
            return m
        grids = config.levels_2d(par, run) if run.ndim == 2 else config.levels(par, run)      # by the file's table: Nx3 = 1 is a 2-D Mesh
        head["levels"] = restart.index_sections(head, [g.Nx for g in grids], run.nscal, run.ion)
        m = cls(lib.Mesh(grids, device, strict, initial=False, nslab=nslab, cuts=cuts), run)
        with open(path, "rb") as f:
            f.seek(head["offset"])
            for g in m.mesh.lev:
                g.read_rst_payload(f)
        m._resumed(head, par)
        return m

    def _set_state(self, time, dt, nstep): self.mesh.set_state(time, dt, nstep)

    time = property(lambda s: s.mesh.time)
    dt = property(lambda s: s.mesh.dt)
    nstep = property(lambda s: s.mesh.nstep)

    def start(self):
        if self.restarted:
            self.mesh.resume()
        else:
            self.mesh.start()

    def step(self): return self.mesh.step()

    def may_batch(self) -> bool:
        """whether advance() may take several steps in one call (outputs.run asks on every pass): a Mesh of 2-D Grids whose steps
        queue with one clock on the device for all levels (aa_mesh_run_2d; lib.Mesh.can_run_2d), or a one-process Mesh of 3-D Grids
        whose levels are all on the queued hydro chain (aa_mesh_run_3d; lib.Mesh.can_run_3d)"""
        return ((hasattr(self.mesh, "can_run_2d") and self.mesh.can_run_2d())
                or (hasattr(self.mesh, "can_run_3d") and self.mesh.can_run_3d()))

    def hst_route(self):
        """None where advance(..., hst=) makes the rows of a history block on the device; else (kind, reason)"""
        if not hasattr(self.mesh, "run_hst_arm"):
            return ("engine", "this engine keeps no state on a device")
        if getattr(self.mesh, "cuts", None) is not None or getattr(self.mesh, "links", None) is not None:
            return ("slabs", "a Mesh cut into slabs steps one at a time")
        return None

    def write_history_rows(self, out, outputs) -> int:
        """the rows the last advance(..., hst=) made: row by row every Domain the block asks for (_fires), as write_history
        visits them -> the number of rows (of each Grid)"""
        rows, _ = self.mesh.run_hst_rows()
        n = len(rows[0]) if rows else 0
        for i in range(n):
            for g, r, (l, d) in zip(self.mesh.lev, rows, self.mesh.domain_numbers()):
                if _fires(out, l, d):
                    self._history_row((out.n, l, d), outputs.dir, l, d, out, outputs, r[i][2:], self._domain_volume(g.cfg.Nx, l),
                                      time=float(r[i][0]), dt=float(r[i][1]))
        return n

    def advance(self, t_stop: float, nstep_stop=None, hst=None) -> int:
        """Whole passes of the main loop until time >= t_stop or nstep == nstep_stop (None: no such limit) as queued steps with one
        read-back per batch (aa_mesh_run_2d / aa_mesh_run_3d); the same bits as that many step() calls.  hst = (t_next, dt_out,
        nlim), where hst_route() is None: history rows of every Grid behind the steps that have one due (write_history_rows).
        -> the steps taken"""
        far = self.nstep + (1 << 20)              # (a call covers 2^20 steps at the most; the caller's loop goes on)
        if hst is not None:
            self.mesh.run_hst_arm(*hst)
        run = self.mesh.run_2d if hasattr(self.mesh, "can_run_2d") and self.mesh.can_run_2d() else self.mesh.run_3d
        return run(t_stop, self.run.tlim, far if nstep_stop is None else min(int(nstep_stop), far))

    def single_route(self, outputs):
        return "a refined mesh (MeshRun) writes no single-variable outputs: they are built for a single-level run"

    def write_dump(self, out, outputs):
        if getattr(outputs, "overlap", False):    # every level's Grid with its own snapshot slots; a level without the route writes now
            t, dt = self.time, self.dt
            for g, (l, d) in zip(self.mesh.lev, self.mesh.domain_numbers()):
                if _fires(out, l, d):
                    rel = dumps.fname(outputs.basename, l, d, out.num, out.out_fmt)
                    if not outputs.overlapped_dump(g, rel, out.out_fmt, out.prim, level=l, domain=d, time=t, dt=dt):
                        g.write_dump(outputs.path(rel), out.out_fmt, out.prim, level=l, domain=d, time=t, dt=dt)
            return
        for rel in self.mesh.write_dump(outputs.dir, outputs.basename, out.num, out.out_fmt, out.prim, out.level, out.domain):
            outputs.written.append(rel)

    def write_history(self, out, outputs):
        for g, (l, d) in zip(self.mesh.lev, self.mesh.domain_numbers()):
            if _fires(out, l, d):
                self._history_row((out.n, l, d), outputs.dir, l, d, out, outputs, g.history(), self._domain_volume(g.cfg.Nx, l))

    def write_restart(self, out, outputs):
        """one file for all levels (restart.c:531-770), the sections of every level from the device in file order"""
        if getattr(outputs, "rst_mesh_ngrid", None):
            if getattr(outputs, "overlap_rst", False):
                outputs.overlap_fallback("rst_ngrid", "restart dumps cut for other Grids (rst_mesh_ngrid) take the boxes of "
                                         "aa_rst_section_get_box", "overlap_rst")
            if getattr(self.mesh, "cuts", None) is not None:
                raise ValueError("[dump_restart]: rst_mesh_ngrid on a Mesh cut into slabs inside the library: its level handles "
                                 "hand out whole sections only")
            lev = self.mesh.lev
            return self._write_restart_mesh_split(out, outputs, [g.cfg.Nx for g in lev],
                                                  lambda n, f, lo, nx: lev[n].write_rst_box_payload(f, lo, nx))
        if getattr(outputs, "overlap_rst", False):    # one job with the snapshot of every level, root first
            rel = dumps.fname(outputs.basename, 0, 0, out.num, "rst")
            if outputs.overlapped_restart(list(self.mesh.lev), rel, self.nstep, self.time, self.dt):
                return
        with self._rst_file(out, outputs) as f:
            for g in self.mesh.lev:
                g.write_rst_payload(f)


# ==================================================================================================
# Static mesh refinement over several GPUs
# ==================================================================================================
class HipMeshEngine:
    """One rank's stack of x3 slabs (one per level present on the rank) on one MI355X."""

    def __init__(self, cfg, device: int = 0, strict: Optional[bool] = None, use_torch_stream: bool = True,
                 initial: bool = True):
        """initial = False: no problem generator, the state of every level comes from a restart dump (lib.Mesh)"""
        import torch
        from . import lib
        self.torch = torch
        self.cfg = cfg
        torch.cuda.set_device(device)
        self.mesh = lib.Mesh(cfg.levels, device, strict, links=cfg.links, initial=initial)
        if use_torch_stream:
            self.mesh.set_stream(torch.cuda.current_stream().cuda_stream)
        self.lev = self.mesh.lev
        dev = torch.device("cuda", device)
        self.scalar_device = dev
        self.send = [[torch.empty(g.halo_doubles(), dtype=torch.float64, device=dev) for _ in range(2)] for g in self.lev]
        self.recv = [[torch.empty(g.halo_doubles(), dtype=torch.float64, device=dev) for _ in range(2)] for g in self.lev]
        self._fbuf = {}
        # one-kernel radiation sub-cycle (levels with rays of 48 zones or more): this rank's reduction words of the level
        # being stepped, and those of all ranks, in device memory
        self.words = torch.zeros(lib.ION_WORDS, dtype=torch.float64, device=dev)
        self.words_all = torch.zeros(lib.ION_WORDS * max(1, cfg.nranks), dtype=torch.float64, device=dev)
        self.neutral = torch.tensor([1.7976931348623157e308, 1.7976931348623157e308, 0, 0, 0, 0, 0, 0], dtype=torch.float64, device=dev)

    nlev = property(lambda s: len(s.lev))

    # per-level slab arithmetic
    def bvals_local(self, l): self.lev[l].bvals_mhd()
    def bvals_ionrad(self, l): self.lev[l].bvals_ionrad()
    def integrate(self, l): self.lev[l].integrate()
    def userwork(self, l): self.lev[l].apply_pinned_cells()
    def ion_begin(self, l): self.lev[l].ion_begin()
    def ion_speculate(self, l, limit): self.lev[l].ion_speculate(limit)
    def ion_rates(self, l): return self.lev[l].ion_rates()
    def ion_update(self, l, dt): return self.lev[l].ion_update(dt)
    def ion_is_fused(self, l): return self.lev[l].ion_is_fused()
    def ion_pass(self, l, update, sweep): self.lev[l].ion_pass(update, sweep, self.words.data_ptr())
    def ion_neutral_words(self): self.words.copy_(self.neutral)          # a rank that holds no zones of the level

    def ion_gather(self, dist):
        """all ranks' words of the level being stepped -> self.words_all (device); one collective per sub-cycle"""
        if dist is None:
            self.words_all[:self.words.numel()].copy_(self.words)
        elif dist.get_backend() == "gloo":                       # rehearsal on one GPU: gloo moves host tensors
            w = self.words.cpu(); wa = self.words_all.cpu()
            dist.all_gather_into_tensor(wa, w)
            self.words_all.copy_(wa)
        else:
            dist.all_gather_into_tensor(self.words_all, self.words)

    def ion_pick(self, l, nranks, first, limit): self.lev[l].ion_pick(self.words_all.data_ptr(), nranks, first, limit)
    def ion_fetch(self, l): return self.lev[l].ion_fetch()
    def ion_finish(self, l): self.lev[l].ion_finish()
    def set_level_state(self, l, time, dt, nstep): self.lev[l].set_mesh_state(time, dt, nstep)
    def cfl_max_v(self, l): return self.lev[l].cfl_max_v()
    def has_radiation(self) -> bool: return bool(self.cfg.levels[0].run.ion)

    # x3 halo of level l
    def pack_x3(self, l, side):
        self.lev[l].pack_x3(side, self.send[l][side].data_ptr()); return self.send[l][side]

    def recv_buffer(self, l, side): return self.recv[l][side]
    def unpack_x3(self, l, side): self.lev[l].unpack_x3(side, self.recv[l][side].data_ptr())

    # level coupling inside the rank
    def restrict_correct_pair(self, l): self.mesh.restrict_correct_pair(l)
    def ion_restrict_correct(self): self.mesh.ionradRestrictCorrect()
    def prolongate(self): self.mesh.Prolongate()
    def ionflux_prolong(self, l): self.mesh.ionflux_prolong(l)

    # flux correction across a cut
    def flux_buffer(self, n1, n2, side=0):
        key = (n1, n2, side)
        if key not in self._fbuf:
            self._fbuf[key] = self.torch.empty(n1 * n2 * 6, dtype=self.torch.float64, device=self.scalar_device)
        return self._fbuf[key]

    def flux_x3_export(self, l, side):
        g = self.lev[l]; nx = self.cfg.levels[l].Nx
        t = self.torch.empty((nx[0] // 2) * (nx[1] // 2) * 6, dtype=self.torch.float64, device=self.scalar_device)
        g.flux_x3_export(side, t.data_ptr()); return t

    def flux_x3_apply(self, l, side, i0, j0, n1, n2, t): self.lev[l].flux_x3_apply(side, i0, j0, n1, n2, t.data_ptr())

    def download(self, l) -> np.ndarray: return self.lev[l].download()
    def edgeflux(self, l) -> np.ndarray: return self.lev[l].download_edgeflux()
    def history(self, l) -> np.ndarray: return self.lev[l].history()
    def set_mesh_state(self, time, dt, nstep): self.mesh.set_state(time, dt, nstep)

    def write_dump(self, rundir, basename, num, fmt, prim, level, domain, time, dt):
        """dump_vtk / dump_binary of every slab of this rank's stack: the payloads come from the device (csrc/dump.hip)"""
        return self.mesh.write_dump(rundir, basename, num, fmt, prim, level, domain, time=time, dt=dt)

    def write_rst_payload(self, l, f): self.lev[l].write_rst_payload(f)
    def read_rst_payload(self, l, f): self.lev[l].read_rst_payload(f)
    def read_rst_boxes(self, l, sources, Nx, lo, n): self.lev[l].read_rst_boxes(sources, Nx, lo, n)
    def write_rst_box_payload(self, l, f, lo, n): self.lev[l].write_rst_box_payload(f, lo, n)
    def sync(self): self.lev[0].sync()
    def close(self): self.mesh.close()


class MeshDriver(_Runner):
    """main() of the reference built with STATIC_MESH_REFINEMENT (main.c:395-447, :519-669) for one
    process of an N-process run in which every level is cut into x3 slabs at the same root planes
    (config.mesh_slabs).  Inside a rank the level coupling is the local aa_mesh; across ranks go the
    x3 halo of every level, the flux correction of a parent plane that lies across a cut from the
    child's boundary, and the scalar reductions (the MPI calls of smr.c, bvals_mhd.c, new_dt.c and
    ionrad_3d.c in the reference)."""

    def __init__(self, par, run: RunConfig, engine_factory=None, rank: int = 0, nranks: int = 1, device: int = 0,
                 strict: Optional[bool] = None, cuts=None, initial: bool = True):
        """initial = False: the product engine skips the problem generator (from_restart loads the state)"""
        self.run, self.rank, self.nranks = run, rank, nranks
        config.check_fofc(run, nranks, mesh=True)
        config.check_2d(run, nranks, mesh=True)
        config.check_1d(run, nranks, mesh=True)
        self.cfg = config.mesh_slabs(par, run, rank, nranks, cuts)
        self.domains = config.levels(par, run)            # the whole Domain of every level (history: its volume)
        self.level_nx1 = [g.Nx[0] for g in self.domains]  # zones along the rays of every level (x3 slabs keep them)
        self.eng = engine_factory(self.cfg) if engine_factory else HipMeshEngine(self.cfg, device, strict, initial=initial)
        self.restarted = False    # from_restart: start() is the restarted run's, outputs.run skips the forced first output
        self.par = None           # the parameter table this driver was built from (from_restart)
        self._hst = {}            # HistoryWriter per (<outputN> block, level)
        self.NL = len(self.cfg.table[0])                  # levels of the Mesh
        self.nl = len(self.cfg.levels)                    # levels present on this rank
        self.time, self.dt, self.nstep = 0.0, 0.0, 0
        self.dtl = [0.0] * self.NL                        # pGrid->dt of every level
        self.tcoarse = 0.0
        self._init_collectives(rank, nranks)
        self.niter_trace: List[List[int]] = []
        self._fused_cache = {}

    def has(self, l: int) -> bool: return l < self.nl

    @classmethod
    def from_restart(cls, path: str, overrides=(), problem: Optional[str] = None, integrator: str = "ctu", order: int = 2,
                     engine_factory=None, rank: int = 0, nranks: int = 1, device: int = 0, strict: Optional[bool] = None,
                     cuts=None, regrid: bool = False) -> "MeshDriver":
        """``athena -r path [block/key=value ...]`` of the MPI + SMR build (main.c:168-173, :216-288; restart_grids,
        restart.c:52-456).  `path` is rank 0's file: every rank takes the parameter table from it, with the overrides on top
        (an unknown key is an error), and reads the Grids it holds, root first, from restart.rank_path(path, rank).  A file
        written for other cuts or another number of ranks holds Grids of other sizes and is refused by the size check of
        restart.index_sections.  The problem generator does not run.  The driver keeps the table as `.par`:
        OutputSet.from_par(d.par, d.time, rundir, rank, nranks) continues the numbering of every <outputN> block.

        regrid = True resumes on THIS driver's slabs (rank, nranks, cuts) whatever cuts wrote the files -- every <domainN> by its
        own NGrid_x1/2/3, x1 cuts included, the Grids dealt to the ranks as restart.mesh_grid_boxes states it: every rank reads,
        for each Grid of its slab stack, the box ``g.disp - domain.disp`` of that level's Domain from every source Grid that
        meets it; time, dt and nstep are rank 0's file's.  `.par` then names the new decomposition (NGrid_x3 of a <domainN> =
        the ranks that hold zones of it, no AutoWithNProc)."""
        head0, par, run = cls._resume_head(path, overrides, problem, integrator, order)
        sources = cls._mesh_sources(head0, par, run)[1] if regrid else None
        d = cls(par, run, engine_factory, rank, nranks, device, strict, cuts, initial=False)
        if not regrid:
            d._resumed(d._read_rank_file(head0, [g.Nx for g in d.cfg.levels], per_level=True), par)
            return d
        for l, g in enumerate(d.cfg.levels):
            dom = d.domains[l]
            lo = tuple(g.disp[a] - (dom.disp[a] if dom.level else 0) for a in range(3))
            if hasattr(d.eng, "read_rst_boxes"):
                d.eng.read_rst_boxes(l, sources[l], dom.Nx, lo, g.Nx)
            elif hasattr(d.eng, "load_state"):
                d.eng.load_state(l, *restart.read_state_boxes(sources[l], dom.Nx, lo, g.Nx, run.nscal))
            else:
                raise RuntimeError("[restart_grids]: this engine takes no state (read_rst_boxes or load_state)")
        held = [sum(1 for r in range(nranks) if d.cfg.table[r][l] is not None) for l in range(d.NL)]
        d._resumed(head0, restart.regrid_mesh_par(par, [(1, 1, n) for n in held]))
        return d

    def _set_state(self, time, dt, nstep):
        self.time, self.dt, self.nstep = time, dt, nstep
        self.dtl = [dt] * self.NL
        if hasattr(self.eng, "set_mesh_state"):
            self.eng.set_mesh_state(time, dt, nstep)
        for l in range(self.nl):
            self.eng.set_level_state(l, time, dt, nstep)

    # ---- outputs (output.c:498-569; outputs.OutputSet drives these) -----------------------------
    def single_route(self, outputs):
        return "a refined mesh over ranks (MeshDriver) writes no single-variable outputs: they are built for a single-level run"

    def write_dump(self, out, outputs):
        """dump_vtk / dump_binary under MPI + SMR: one file per level this rank holds zones of, under the rank's directory;
        the header is the slab's own (its DIMENSIONS and ORIGIN, the level's spacing, the Mesh time)."""
        if getattr(outputs, "overlap", False):
            outputs.overlap_fallback("MeshDriver", "overlapped dumps are not built for a refined mesh over several ranks (MeshDriver)")
        if hasattr(self.eng, "write_dump"):
            for rel in self.eng.write_dump(outputs.dir, outputs.basename, out.num, out.out_fmt, out.prim, out.level, out.domain,
                                           self.time, self.dt):
                outputs.written.append(rel)
            return
        ng, r = config.NGHOST, self.run
        for l, g in enumerate(self.cfg.levels):   # an engine without a device: the same payload from its host blocks
            if not _fires(out, l):
                continue
            path = outputs.path(dumps.fname(outputs.basename, l, 0, out.num, out.out_fmt))
            U = self.eng.download(l)[ng:-ng, ng:-ng, ng:-ng]
            dumps.write_dump_from_block(path, out.out_fmt, U, prim=out.prim, gamma=r.gamma, nscal=r.nscal, nx=g.Nx,
                                        minx=g.MinX, dx=tuple(r.dx[a] / float(1 << l) for a in range(3)), time=self.time,
                                        dt=self.dt, level=l, domain=0)

    def history(self) -> np.ndarray:
        """dump_history.c:157-260 for every level: [NL][9] volume integrals, each level's added over the ranks that hold
        zones of it (MPI_Reduce(SUM) :257 over the Domain's communicator; here ONE all-reduce for all levels, in which a
        rank without the level takes part with zeros)."""
        s = np.zeros((self.NL, 9))
        for l in range(self.nl):
            s[l] = self.eng.history(l)
        if self.distributed:
            s = np.array(self._allreduce(s.reshape(-1), self.dist.ReduceOp.SUM)).reshape(self.NL, 9)
        return s

    def hst_route(self):
        """(kind, reason): outputs.run with hst_queued keeps the history block a stop time here"""
        return ("MeshDriver", "a MeshDriver steps its ranks' slabs one at a time and adds their rows on the host")

    def write_history(self, out, outputs):
        """One row per level.  The sums are divided by the volume of the whole Domain (:271-279); the lowest rank that holds
        zones of a level writes its file, under rank 0's directory with its OWN problem_id in the name (:328-349)."""
        s = self.history()                         # (every rank takes part in the sum)
        id0 = os.path.join(os.path.dirname(outputs.dir), "id0") if outputs.nranks > 1 else outputs.dir
        for l, g in enumerate(self.domains):
            if _fires(out, l) and self.rank == min(r for r in range(self.nranks) if self.cfg.table[r][l] is not None):
                self._history_row((out.n, l), id0, l, 0, out, outputs, s[l], self._domain_volume(g.Nx, l))

    def write_restart(self, out, outputs):
        """dump_restart (restart.c:463-983): ONE file per rank -- the parameter table as it stands now, then the sections of
        every Grid this rank holds, root first (:531-770)."""
        if getattr(outputs, "overlap_rst", False):
            outputs.overlap_fallback("MeshDriver", "overlapped restart dumps are not built for a refined mesh over several ranks "
                                     "(MeshDriver)", "overlap_rst")
        if getattr(outputs, "rst_mesh_ngrid", None):
            return self._write_restart_split(out, outputs)
        with self._rst_file(out, outputs) as f:
            for l in range(self.nl):
                if hasattr(self.eng, "write_rst_payload"):    # the sections come from the device in file order (csrc/restart.hip)
                    self.eng.write_rst_payload(l, f)
                else:
                    restart.write_grid_sections(f, *self._host_state(l))

    def _write_restart_split(self, out, outputs):
        """OutputSet(rst_mesh_ngrid=...) on one rank, whose slab stack is every whole Domain (_Runner._write_restart_mesh_split)"""
        if self.nranks > 1:
            raise ValueError("[dump_restart]: rst_mesh_ngrid takes a one-rank run")
        if hasattr(self.eng, "write_rst_box_payload"):
            def payload(l, f, lo, nx): self.eng.write_rst_box_payload(l, f, lo, nx)
        else:
            host = {}

            def payload(l, f, lo, nx):
                if l not in host:
                    host.clear()                      # (one level's host block at a time)
                    host[l] = self._host_state(l)
                U, ef = host[l]
                k, j, i = (slice(lo[a], lo[a] + nx[a]) for a in (2, 1, 0))
                k1, j1, i1 = (slice(lo[a], lo[a] + nx[a] + 1) for a in (2, 1, 0))
                restart.write_grid_sections(f, U[k, j, i], None if ef is None else ef[k1, j1, i1])
        self._write_restart_mesh_split(out, outputs, [g.Nx for g in self.domains], payload)

    def _p2p(self, sends, recvs):
        """sends: [(tensor, peer)], recvs: [(tensor, peer)]; gloo moves host tensors only."""
        dist = self.dist
        host_stage = (dist.get_backend() == "gloo")
        ops, staged = [], []
        for t, peer in sends:
            ops.append(dist.P2POp(dist.isend, t.cpu() if (host_stage and t.is_cuda) else t, peer))
        for t, peer in recvs:
            if host_stage and t.is_cuda:
                h = self.torch.empty(t.shape, dtype=t.dtype); staged.append((t, h)); t = h
            ops.append(dist.P2POp(dist.irecv, t, peer))
        if ops:
            for w in dist.batch_isend_irecv(ops):
                w.wait()
        for t, h in staged:
            t.copy_(h)

    # ---- ghost zones ---------------------------------------------------------------------------
    def exchange_x3(self, l: int):
        if not self.distributed or not self.has(l):
            return
        g, e = self.cfg.levels[l], self.eng
        if g.lx3 < 0 and g.rx3 < 0:
            return
        sends, recvs, sides = [], [], []
        if g.lx3 == g.rx3 and g.lx3 >= 0:
            # two slabs with periodic wrap: post so that the peer's inner planes land in my OUTER ghosts
            sends = [(e.pack_x3(l, 0), g.lx3), (e.pack_x3(l, 1), g.rx3)]
            recvs = [(e.recv_buffer(l, 1), g.rx3), (e.recv_buffer(l, 0), g.lx3)]
            sides = [0, 1]
        else:
            if g.lx3 >= 0:
                sends.append((e.pack_x3(l, 0), g.lx3)); recvs.append((e.recv_buffer(l, 0), g.lx3)); sides.append(0)
            if g.rx3 >= 0:
                sends.append((e.pack_x3(l, 1), g.rx3)); recvs.append((e.recv_buffer(l, 1), g.rx3)); sides.append(1)
        self._p2p(sends, recvs)
        for side in sides:
            e.unpack_x3(l, side)

    def bvals_mhd(self, l: int):
        if self.has(l):
            self.eng.bvals_local(l)
        self.exchange_x3(l)

    # ---- level coupling ------------------------------------------------------------------------
    def restrict_correct(self):
        """smr.c:1207: finest pair first; a parent plane that lies across a cut from the child's
        boundary is corrected by the rank that owns it, with the child's restricted flux as message."""
        for l in range(self.NL - 2, -1, -1):
            if self.has(l + 1):
                self.eng.restrict_correct_pair(l)
            if not self.distributed:
                continue
            sends, recvs, todo = [], [], []
            if self.has(l + 1):
                for side, peer in enumerate(self.cfg.links[l].corr_to):
                    if peer >= 0:
                        sends.append((self.eng.flux_x3_export(l + 1, side), peer))
            for (lp, side, src, i0, j0, n1, n2) in self.cfg.corr_in:
                if lp == l:
                    buf = self.eng.flux_buffer(n1, n2, side)
                    recvs.append((buf, src)); todo.append((side, i0, j0, n1, n2, buf))
            self._p2p(sends, recvs)
            for side, i0, j0, n1, n2, buf in todo:
                self.eng.flux_x3_apply(l, side, i0, j0, n1, n2, buf)

    # ---- time step -------------------------------------------------------------------------------
    def new_dt(self):
        """new_dt.c:32 over all levels: max(|v|+a) per level (MAX over its slabs), carried from level to
        level (:33), one dt for the Mesh."""
        v = []
        for l in range(self.NL):
            v += self.eng.cfl_max_v(l) if self.has(l) else [0.0, 0.0, 0.0]
        if self.distributed:
            v = self._allreduce(v, self.dist.ReduceOp.MAX)
        max_dti = fold_levels(v, [[x / float(1 << l) for x in self.run.dx] for l in range(self.NL)])
        self.dt = pick_dt(self.nstep, self.dt, self.run.cour_no / max_dti, self.time, self.run.tlim)
        for l in range(self.NL):
            self.dtl[l] = self.dt
            if self.has(l):
                self.eng.set_level_state(l, self.time, self.dt, self.nstep)

    # ---- radiation ---------------------------------------------------------------------------------
    def _level_fused(self, l: int) -> bool:
        """whether level l runs the one-kernel sub-cycle: asked of the LIBRARY (aa_ion_is_fused: it knows aa_params.ion_path,
        AA_ION_FUSED as it parses it, the ray direction) on the ranks that hold zones of the level, and agreed on by all
        ranks once -- ranks without zones of the level have no Grid to ask, and a rank that disagreed would issue the
        other protocol's collectives."""
        if l in self._fused_cache:
            return self._fused_cache[l]
        if not hasattr(self.eng, "ion_pass") or not hasattr(self.eng, "ion_is_fused"):
            ans = False
        else:
            mine = (1.0 if self.eng.ion_is_fused(l) else 0.0) if self.has(l) else -1.0          # -1: no opinion
            if self.distributed:
                hi = self._allreduce((mine,), self.dist.ReduceOp.MAX)[0]
                lo = self._allreduce((mine if mine >= 0 else 2.0,), self.dist.ReduceOp.MIN)[0]
                if hi >= 0 and lo <= 1.0 and hi != lo:
                    raise RuntimeError(f"[MeshDriver]: the ranks disagree on the radiation sub-cycle path of level {l}")
                ans = hi > 0.5
            else:
                ans = mine > 0.5
        self._fused_cache[l] = ans
        return ans

    def _ion_radtransfer_fused(self, l: int) -> int:
        """ionrad_3d.c:862 on level l with the one-kernel sub-cycle (see Driver._ion_radtransfer_fused): one pass, ONE
        all-gather of the ranks' reduction words and one read-back per sub-cycle.  A rank without zones of the level
        contributes neutral words and follows the control flow from the gathered words (the arithmetic of k_ion_pick2)."""
        e, has = self.eng, self.has(l)
        dist = self.dist if self.distributed else None
        nr = self.nranks if self.distributed else 1
        fine = l != 0
        if fine:
            if has:
                e.ionflux_prolong(l)
        else:
            self.tcoarse = 0.0
        limit = self.tcoarse if fine else self.dtl[0]
        if has:
            e.set_level_state(l, self.time, self.dtl[l], self.nstep)
            e.ion_begin(l)
            if hasattr(e, "ion_speculate"):
                e.ion_speculate(l, limit)      # (see Driver._ion_radtransfer_fused)
        mir = {"dt_sel": 0.0, "hit": False, "neg": False, "dt_done": 0.0}

        def one_pass(update, first):
            if has:
                e.ion_pass(l, update, True)
            else:
                e.ion_neutral_words()
            e.ion_gather(dist)
            if has:
                e.ion_pick(l, nr, first, limit)
                return e.ion_fetch(l) if not first else None
            W = e.words_all.tolist()                                   # this rank's one wait of the sub-cycle
            n = len(W) // nr
            dt_chem = min(W[0::n]); dt_therm = min(W[1::n]); max_dti = max(W[2::n]); count = sum(W[3::n]); neg = max(W[4::n]) != 0.0
            out = None
            if not first:
                out = (mir["dt_sel"], mir["hit"], dt_chem, dt_therm, int(count), self.run.cour_no / max_dti if max_dti > 0 else float("inf"), mir["neg"])
                mir["dt_done"] = mir["dt_done"] + mir["dt_sel"]
            else:
                mir["dt_done"] = 0.0
            mir["dt_sel"], mir["hit"] = pick_step(dt_chem, dt_therm, mir["dt_done"], limit)
            mir["neg"] = neg
            return out

        one_pass(False, True)
        niter, dt_done, cut = subcycles(lambda dt_done: _fetched(one_pass(True, False)), fine)
        if has:
            e.ion_finish(l)
        return self._ion_close(l, niter, dt_done, cut)

    def _ion_close(self, l: int, niter: int, dt_done: float, cut: bool) -> int:
        """what level l's sub-cycle loop leaves behind: its step, the root's closing (ionrad_3d.c:1017-1029, :1044), :1033"""
        if cut:
            self.dtl[l] = dt_done
        if l == 0:
            self.dtl[0], self.tcoarse = close_root(niter, self.run.maxiter, self.dtl[0], dt_done)
        self.dt = self.dtl[l]                                   # ionrad_3d.c:1033 pMesh->dt = pGrid->dt
        if self.has(l):
            self.eng.set_level_state(l, self.time, self.dtl[l], self.nstep)
        return niter

    def ion_radtransfer(self, l: int) -> int:
        """ionrad_3d.c:862 on level l (all ranks take part in the reductions, with neutral values where
        the level is absent)."""
        if self._level_fused(l):
            return self._ion_radtransfer_fused(l)
        e, has = self.eng, self.has(l)
        fine = l != 0
        INF = float("inf")
        if fine:
            if has:
                e.ionflux_prolong(l)
        else:
            self.tcoarse = 0.0
        limit = self.tcoarse if fine else self.dtl[0]
        if has:
            e.set_level_state(l, self.time, self.dtl[l], self.nstep)
            e.ion_begin(l)

        def one(dt_done):
            dt_chem, dt_therm = e.ion_rates(l) if has else (INF, INF)
            if self.distributed:
                dt_chem, dt_therm = self._allreduce((dt_chem, dt_therm), self.dist.ReduceOp.MIN)
            dt, hit = pick_step(dt_chem, dt_therm, dt_done, limit)
            cellcount, dt_hydro = e.ion_update(l, dt) if has else (0, INF)
            if self.distributed and not fine:
                t = self._allreduce((float(cellcount),), self.dist.ReduceOp.SUM)
                h = self._allreduce((dt_hydro,), self.dist.ReduceOp.MIN)
                cellcount, dt_hydro = int(t[0]), h[0]
            return dt, hit, cellcount, dt_hydro

        niter, dt_done, cut = subcycles(one, fine)
        return self._ion_close(l, niter, dt_done, cut)

    # ---- main.c ----------------------------------------------------------------------------------------
    def start(self):
        for l in range(self.nl):
            self.eng.set_level_state(l, self.time, 0.0, self.nstep)
        self.restrict_correct()
        for l in range(self.NL):
            self.bvals_mhd(l)
            if self.has(l):
                self.eng.bvals_ionrad(l)
        self.eng.prolongate()
        if self.restarted:          # main.c:398-451 after restart_grids: NO new_dt -- the file's dt is the next step's
            for l in range(self.NL):
                self.dtl[l] = self.dt
                if self.has(l):
                    self.eng.set_level_state(l, self.time, self.dt, self.nstep)
        else:
            self.new_dt()
        return self

    def step(self) -> List[int]:
        niter = [0] * self.NL
        if self.eng.has_radiation():                              # main.c:546-562
            for l in range(self.NL):
                niter[l] = self.ion_radtransfer(l)
                self.bvals_mhd(l)
            self.eng.ion_restrict_correct()
        for l in range(self.nl):                                  # :572-585
            self.eng.set_level_state(l, self.time, self.dtl[l], self.nstep)
            self.eng.integrate(l)
        self.restrict_correct()                                   # :591
        for l in range(self.nl):                                  # :597
            self.eng.userwork(l)
        self.nstep += 1
        self.time += self.dt                                      # :618-626
        self.new_dt()                                             # :629
        for l in range(self.NL):                                  # :635-644
            self.bvals_mhd(l)
        self.eng.prolongate()                                     # :647
        self.niter_trace.append(niter)
        return niter
