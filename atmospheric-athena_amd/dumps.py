"""Data dumps of the reference: ``out_fmt = vtk`` (dump_vtk.c:28-327) and ``out_fmt = bin`` (dump_binary.c:30-266), with
``out = cons`` or ``out = prim``.

Both formats are single precision over the ACTIVE zones of one Grid.  A file is a header (text for vtk, a small binary
record for bin) around *sections* of field data, zones ``[k][j][i]`` with i fastest:

  vtk: ``density`` (n floats) | ``momentum`` / ``velocity`` (3n, the components of a zone next to each other) |
       ``total_energy`` / ``pressure`` (n) | ``scalar[s]`` / ``specific_scalar[s]`` (n each); big-endian words
  bin: NVAR = 5 + NSCALARS sections of n floats in ConsS / PrimS order; native (little-endian) words

The writers take the sections from a callable, so the device path (``lib.Grid.dump_section``: the payload is made by the
kernel of csrc/dump.hip and arrives in file order and byte order) and the host path (``payload_from_block``: the same
arithmetic in numpy, for engines without a device and as the checker of the kernel) share every byte of header.
"""
from __future__ import annotations

import collections
import os
import struct
import threading
from typing import Callable, List, Optional, Sequence

import numpy as np

VTK, BIN = 1, 2                      # AA_DUMP_VTK / AA_DUMP_BIN of include/athena_amd.h
FORMATS = {"vtk": VTK, "bin": BIN}
TINY_NUMBER = 1.0e-20                # defs.h.in:160
NUM_DIGIT = 4                        # the reference's num_digit


def nsections(fmt: int, nscal: int) -> int:
    return (3 if fmt == VTK else 5) + nscal


def section_floats(fmt: int, section: int, nzones: int) -> int:
    return 3 * nzones if (fmt == VTK and section == 1) else nzones


def payload_from_block(U: np.ndarray, fmt: int, prim: bool, gamma: float, nscal: Optional[int] = None) -> List[np.ndarray]:
    """The sections of a dump from a host block of ACTIVE zones ``[k][j][i][var]`` (d, M1, M2, M3, E[, s0]), each a flat
    array in the file's dtype.  Primitive variables operation by operation as Cons1D_to_Prim1D (convert_var.c:389-421):
    ``di = 1/d``, ``V = M*di``, ``P = MAX((E - 0.5*(M1^2 + M2^2 + M3^2)*di)*Gamma_1, TINY_NUMBER)`` -- the macro sends a
    NaN to TINY_NUMBER -- and ``r = s*di``."""
    fmt = FORMATS.get(fmt, fmt)
    nscal = U.shape[-1] - 5 if nscal is None else nscal
    dt = ">f4" if fmt == VTK else "<f4"
    d, M1, M2, M3, E = (U[..., c] for c in range(5))
    with np.errstate(all="ignore"):
        if prim:
            di = 1.0 / d
            P = E - 0.5 * (M1 * M1 + M2 * M2 + M3 * M3) * di
            P = P * (gamma - 1.0)
            P = np.where(P > TINY_NUMBER, P, TINY_NUMBER)
            v = [d, M1 * di, M2 * di, M3 * di, P] + [U[..., 5 + s] * di for s in range(nscal)]
        else:
            v = [d, M1, M2, M3, E] + [U[..., 5 + s] for s in range(nscal)]
        if fmt == VTK:
            v = [v[0], np.stack(v[1:4], axis=-1), v[4]] + v[5:]
        return [np.ascontiguousarray(a).astype(dt).reshape(-1) for a in v]


def fname(basename: str, level: int, domain: int, num: int, ext: str) -> str:
    """ath_fname(plev, basename, plev, pdom, num_digit, num, NULL, ext) (ath_files.c:41-130), relative to the run directory."""
    name = basename + (f"-lev{level}" if level > 0 else "") + (f"-dom{domain}" if domain > 0 else "")
    name += ".%0*d.%s" % (NUM_DIGIT, num, ext)
    return os.path.join(f"lev{level}", name) if level > 0 else name


def vtk_titles(prim: bool, nscal: int) -> List[bytes]:
    """The text in front of every section (dump_vtk.c:164-301): every title but the first begins with a newline."""
    t = [b"SCALARS density float\nLOOKUP_TABLE default\n",
         b"\nVECTORS velocity float\n" if prim else b"\nVECTORS momentum float\n",
         (b"\nSCALARS pressure float\n" if prim else b"\nSCALARS total_energy float\n") + b"LOOKUP_TABLE default\n"]
    for s in range(nscal):
        t.append((b"\nSCALARS specific_scalar[%d] float\n" if prim else b"\nSCALARS scalar[%d] float\n") % s
                 + b"LOOKUP_TABLE default\n")
    return t


def vtk_header(nx: Sequence[int], minx: Sequence[float], dx: Sequence[float], time: float, level: int, domain: int,
               prim: bool) -> bytes:
    """dump_vtk.c:121-160: DIMENSIONS counts the zone CORNERS (1 along x3 on a 2-D Grid, 1 along x2 and x3 on a 1-D Grid, :146-152),
    the ORIGIN / SPACING / CELL_DATA lines end in a blank."""
    s = "# vtk DataFile Version 2.0\n"
    s += "%s vars at time= %e, level= %i, domain= %i\n" % ("PRIMITIVE" if prim else "CONSERVED", time, level, domain)
    s += "BINARY\nDATASET STRUCTURED_POINTS\n"
    s += "DIMENSIONS %d %d %d\n" % (nx[0] + 1, nx[1] + 1 if nx[1] > 1 else 1, nx[2] + 1 if nx[2] > 1 and nx[1] > 1 else 1)
    s += "ORIGIN %e %e %e \n" % (minx[0], minx[1], minx[2])
    s += "SPACING %e %e %e \n" % (dx[0], dx[1], dx[2])
    s += "CELL_DATA %d \n" % (nx[0] * nx[1] * nx[2])
    return s.encode()


def bin_header(nx: Sequence[int], minx: Sequence[float], dx: Sequence[float], time: float, dt: float, gamma: float,
               nscal: int) -> bytes:
    """dump_binary.c:111-191: coordsys = -1 (Cartesian), ndata[7] = zones, NVAR, NSCALARS, no self-gravity, no particles;
    (float)Gamma_1 and 0 (adiabatic); (float)time, (float)dt; the zone centres along x1, x2, x3 (cc_pos.c:36-43) as floats."""
    b = struct.pack("<i7i", -1, nx[0], nx[1], nx[2], 5 + nscal, nscal, 0, 0)
    b += np.array([gamma - 1.0, 0.0], dtype="<f4").tobytes()
    b += np.array([time, dt], dtype="<f4").tobytes()
    for a in range(3):
        x = minx[a] + (np.arange(nx[a], dtype=np.float64) + 0.5) * dx[a]
        b += x.astype("<f4").tobytes()
    return b


def _raw(a) -> memoryview:
    a = np.ascontiguousarray(a)
    return memoryview(a).cast("B")


def dump_head(fmt, *, nx, minx, dx, time: float, dt: float, gamma: float, prim: bool, nscal: int, level: int = 0,
              domain: int = 0):
    """-> (header bytes, [the bytes in front of section i]) of a dump file: everything in it that is not field data.  vtk: the
    text header and the title lines of every section; bin: the binary header, nothing between the sections.  (`prim` does not
    show in a bin file: the reference's header does not say which set it holds.)"""
    fmt = FORMATS.get(fmt, fmt)
    if fmt == VTK:
        return vtk_header(nx, minx, dx, time, level, domain, prim), vtk_titles(prim, nscal)
    if fmt == BIN:
        return bin_header(nx, minx, dx, time, dt, gamma, nscal), [b""] * (5 + nscal)
    raise ValueError(f"[write_dump]: format {fmt!r} (vtk or bin)")


def write_sections(path: str, header: bytes, titles: Sequence[bytes], section: Callable[[int], np.ndarray],
                   trailer: bytes = b"") -> None:
    """header | title 0 | section(0) | title 1 | section(1) ... | trailer: the one place that lays a dump file out"""
    with open(path, "wb") as f:
        f.write(header)
        for i, title in enumerate(titles):
            if title:
                f.write(title)
            f.write(_raw(section(i)))
        if trailer:
            f.write(trailer)


def write_vtk(path: str, section: Callable[[int], np.ndarray], *, nx, minx, dx, time: float, prim: bool, nscal: int,
              level: int = 0, domain: int = 0) -> None:
    """``section(i)`` returns section i of the vtk payload (big-endian words, see the module text), as an array or bytes."""
    write_sections(path, vtk_header(nx, minx, dx, time, level, domain, prim), vtk_titles(prim, nscal), section)


def write_bin(path: str, section: Callable[[int], np.ndarray], *, nx, minx, dx, time: float, dt: float, gamma: float,
              prim: bool, nscal: int) -> None:
    """``section(i)`` returns variable i of the bin payload (native words).  (`prim` does not show in the file: the reference's
    header does not say which set it holds.)"""
    write_sections(path, bin_header(nx, minx, dx, time, dt, gamma, nscal), [b""] * (5 + nscal), section)


def write_dump(path: str, fmt, section: Callable[[int], np.ndarray], *, nx, minx, dx, time: float, dt: float, gamma: float,
               prim: bool, nscal: int, level: int = 0, domain: int = 0) -> None:
    fmt = FORMATS.get(fmt, fmt)
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    if fmt == VTK:
        write_vtk(path, section, nx=nx, minx=minx, dx=dx, time=time, prim=prim, nscal=nscal, level=level, domain=domain)
    elif fmt == BIN:
        write_bin(path, section, nx=nx, minx=minx, dx=dx, time=time, dt=dt, gamma=gamma, prim=prim, nscal=nscal)
    else:
        raise ValueError(f"[write_dump]: format {fmt!r} (vtk or bin)")


def write_dump_from_block(path: str, fmt, U: np.ndarray, *, prim: bool, gamma: float, nscal: int, **kw) -> None:
    """A dump of a host block of active zones (the CPU engines' path)."""
    pay = payload_from_block(U, fmt, prim, gamma, nscal)
    write_dump(path, fmt, lambda i: pay[i], prim=prim, gamma=gamma, nscal=nscal, **kw)


# ---- single-variable outputs: output_vtk.c, output_tab.c, output_pgm.c around the payload of OutData1/2/3 (output.c:629-1107) ----
EXPR = {"d": 0, "M1": 1, "M2": 2, "M3": 3, "E": 4, "V1": 5, "V2": 6, "V3": 7, "P": 8, "cs2": 9, "flux": 10}    # AA_OUT_*
FLT_EPSILON = float(np.finfo(np.float32).eps)


def fname_id(basename: str, level: int, domain: int, num: int, id_: str, ext: str) -> str:
    """ath_fname(plev, basename, plev, pdom, num_digit, num, id, ext): ``<base>.NNNN.<id>.<ext>``"""
    name = basename + (f"-lev{level}" if level > 0 else "") + (f"-dom{domain}" if domain > 0 else "")
    name += ".%0*d.%s.%s" % (NUM_DIGIT, num, id_, ext)
    return os.path.join(f"lev{level}", name) if level > 0 else name


def expr_from_block(U: np.ndarray, expr: str, gamma: float, edgeflux: Optional[np.ndarray] = None) -> np.ndarray:
    """expr_* of output.c:1109-1233 over a host block ``[k][j][i][var]``, operation by operation (numpy does not contract);
    flux: the block of EdgeFlux itself (prob/ioniz_sphere.c:356-359)."""
    if expr == "flux":
        return np.asarray(edgeflux, dtype=np.float64)
    d, M1, M2, M3, E = (U[..., c] for c in range(5))
    with np.errstate(all="ignore"):
        if expr in ("d", "M1", "M2", "M3", "E"):
            return np.array(U[..., EXPR[expr]], dtype=np.float64)
        if expr in ("V1", "V2", "V3"):
            return U[..., EXPR[expr] - 4] / d
        e = E - 0.5 * (M1 * M1 + M2 * M2 + M3 * M3) / d
        if expr == "P":
            return (gamma - 1.0) * e
        if expr == "cs2":
            return gamma * (gamma - 1.0) * e / d
    raise ValueError(f"[expr_from_block]: expression {expr!r}")


def outdata_from_values(V: np.ndarray, first, reduce, lo, hi) -> np.ndarray:
    """OutData1/2/3 from the expression's values `V` ``[k][j][i]`` over a block whose zone [first[2]][first[1]][first[0]] is the
    first active one (a block with ghost zones: first = nghost where the direction has them).  Direction a covers the zones
    lo[a] .. hi[a], counted from the first active one: all active zones where it is kept (reduce[a] false), the slice where it is
    summed -- in the reference's order, k, j, i ascending from 0.0, then times 1.0/count/count.  A summed range may reach into
    the ghost zones (see outputs.slice_zones).  -> [n3][n2][n1], a reduced direction with one element."""
    sub = V[first[2] + lo[2]:first[2] + hi[2] + 1, first[1] + lo[1]:first[1] + hi[1] + 1, first[0] + lo[0]:first[0] + hi[0] + 1]
    if not any(reduce):
        return np.ascontiguousarray(sub)
    n = [1 if reduce[a] else sub.shape[2 - a] for a in range(3)]
    acc = np.zeros((n[2], n[1], n[0]))
    factor = 1.0
    for a in (2, 1, 0):
        if reduce[a]:
            factor = factor / float(hi[a] - lo[a] + 1)

    def steps(a):
        return [slice(q, q + 1) for q in range(sub.shape[2 - a])] if reduce[a] else [slice(None)]
    with np.errstate(all="ignore"):
        for sk in steps(2):
            for sj in steps(1):
                for si in steps(0):
                    acc = acc + sub[sk, sj, si]
        return acc * factor


def minmax(data: np.ndarray):
    """minmax1/2/3 (utils.c:142-197): the fold ``dmin = dmin < x ? dmin : x`` in payload order, so that of elements that compare
    equal (zeros of either sign) the last stays"""
    flat = np.asarray(data, dtype=np.float64).reshape(-1)
    mn, mx = flat.min(), flat.max()
    return float(flat[np.nonzero(flat == mn)[0][-1]]), float(flat[np.nonzero(flat == mx)[0][-1]])


def pgm_gray(data2: np.ndarray, dmin: float, dmax: float) -> np.ndarray:
    """output_pgm.c:94-122 for the payload ``[nx2][nx1]``: the bytes in file order"""
    data2 = np.asarray(data2, dtype=np.float64)
    max_min = (dmax - dmin) * (1.0 + FLT_EPSILON)
    if not max_min > 0.0:
        return np.zeros(data2.size, dtype=np.uint8)
    sfact = 256.0 / max_min
    with np.errstate(all="ignore"):
        x = sfact * (data2[::-1, :] - dmin)
        ok = (x > -2147483649.0) & (x < 2147483648.0)        # (int) of a double outside int, or a NaN: INT_MIN on the reference's host
        g = np.where(ok, np.trunc(np.where(ok, x, 0.0)), -2147483648.0)
    return np.clip(g, 0, 255).astype(np.uint8).reshape(-1)


def single_vtk_bytes(data: np.ndarray, id_: str, *, nx, minx, dx, raw_reduce, time: float, level: int = 0, domain: int = 0) -> bytes:
    """output_vtk_2d / output_vtk_3d (output_vtk.c:70-278) for the payload `data` ([nx3][nx2][nx1], or [nx2][nx1] of a 2-D
    output).  nx, minx, dx: the Grid's; raw_reduce: the block's reduce_x1/2/3 as parse_slice set them (SPACING of a reduced
    direction is the Grid's whole extent, :142-144)."""
    data = np.asarray(data)
    s = "# vtk DataFile Version 2.0\n"
    s += "Really cool Athena data at time= %e, level= %i, domain= %i\n" % (time, level, domain)
    s += "BINARY\nDATASET STRUCTURED_POINTS\n"
    if data.ndim == 2:
        n2, n1 = data.shape
        sp = [dx[a] * nx[a] if raw_reduce[a] else dx[a] for a in range(3)]
        s += "DIMENSIONS %d %d %d\n" % (n1 + 1, n2 + 1, 1)
        s += "ORIGIN %e %e %e \n" % (minx[0], minx[1], minx[2])
        s += "SPACING %e %e %e \n" % (sp[0], sp[1], sp[2])
        s += "CELL_DATA %d \n" % (n1 * n2)
    else:
        n3, n2, n1 = data.shape
        s += "DIMENSIONS %d %d %d\n" % (n1 + 1, n2 + 1, n3 + 1)
        s += "ORIGIN %e %e %e \n" % (minx[0], minx[1], minx[2])
        s += "SPACING %e %e %e \n" % (dx[0], dx[1], dx[2])
        s += "CELL_DATA %d \n" % (n1 * n2 * n3)
    s += "SCALARS %s float\nLOOKUP_TABLE default\n" % id_
    with np.errstate(all="ignore"):
        return s.encode() + data.astype(">f4").tobytes()


def single_tab_bytes(data: np.ndarray, dat_fmt: Optional[str] = None) -> bytes:
    """output_tab_1d/2d/3d (output_tab.c:75-283): the zone indices as (float) in the first columns, the value in the last, every
    column through ``" " + dat_fmt`` (default ``%12.8e``)"""
    fmt = " " + (dat_fmt if dat_fmt is not None else "%12.8e")
    data = np.asarray(data, dtype=np.float64)
    nd = data.ndim
    line = fmt * (nd + 1) + "\n"
    out = []
    if nd == 1:
        for i in range(data.shape[0]):
            out.append(line % (float(i), float(data[i])))
    elif nd == 2:
        for j in range(data.shape[0]):
            for i in range(data.shape[1]):
                out.append(line % (float(i), float(j), float(data[j, i])))
    else:
        for k in range(data.shape[0]):
            for j in range(data.shape[1]):
                for i in range(data.shape[2]):
                    out.append(line % (float(i), float(j), float(k), float(data[k, j, i])))
    return "".join(out).encode()


def single_pgm_bytes(gray: np.ndarray, nx1: int, nx2: int) -> bytes:
    """output_pgm.c:83: the header in front of the nx1*nx2 gray bytes (pgm_gray, or the device's)"""
    return b"P5\n%d %d\n255\n" % (nx1, nx2) + np.asarray(gray, dtype=np.uint8).tobytes()


class OverlapWriter:
    """Writes dump files on ONE background thread while the run goes on.  Pure Python: the worker touches nothing but the
    arrays of a job (page-locked host memory that a device copy has filled and finished with) and files -- it never calls the
    library, HIP or torch.  Whatever has to happen on the driving thread when a file is complete (giving the snapshot's slot
    back) is the job's ``on_done``, which `poll`, `wait` and `finish` run on THEIR caller's thread.

    A job is (path, header bytes, section titles, section arrays, on_done[, trailer bytes: what stands behind the last section --
    a restart dump's USER_DATA label]).  The worker writes ``path + ".part"`` and renames it
    onto `path` when the file is complete: a file under its final name is always whole.  Jobs are written in the order of
    `submit`, so of two jobs for the same path the later one stays.  An exception of the worker is kept (the first one, until it
    has been raised; the job's on_done still runs, the jobs behind it are tried all the same), and the next `poll` / `wait` or
    `finish` re-raises it in the driving thread."""

    def __init__(self):
        self._cv = threading.Condition()
        self._jobs = collections.deque()     # submitted, not yet taken by the worker
        self._done = collections.deque()     # (ticket, on_done) of finished jobs whose on_done has not run yet
        self._submitted = 0                  # tickets handed out / jobs the worker is through with
        self._completed = 0
        self._error = None
        self._thread = None
        self._stop = False

    def submit(self, path: str, header: bytes, titles: Sequence[bytes], sections: Sequence[np.ndarray], on_done=None,
               trailer: bytes = b"") -> int:
        """-> the job's ticket (for `wait`)"""
        with self._cv:
            self._submitted += 1
            self._jobs.append((self._submitted, path, header, list(titles), list(sections), on_done, bytes(trailer)))
            if self._thread is None:
                self._stop = False
                self._thread = threading.Thread(target=self._work, name="dump-writer", daemon=True)
                self._thread.start()
            self._cv.notify_all()
            return self._submitted

    def _work(self):
        while True:
            with self._cv:
                while not self._jobs and not self._stop:
                    self._cv.wait()
                if not self._jobs:
                    return
                ticket, path, header, titles, sections, on_done, trailer = self._jobs.popleft()
            err = None
            try:
                write_sections(path + ".part", header, titles, lambda i: sections[i], trailer)
                os.replace(path + ".part", path)
            except BaseException as e:           # kept for the driving thread
                err = e
            del sections
            with self._cv:
                if err is not None and self._error is None:
                    self._error = err
                self._completed = ticket
                self._done.append((ticket, on_done))
                self._cv.notify_all()

    def _settle(self):
        """on the caller's thread: the on_done of every finished job, then the worker's exception if there is one"""
        while True:
            with self._cv:
                if not self._done:
                    break
                _ticket, on_done = self._done.popleft()
            if on_done is not None:
                on_done()
        with self._cv:
            err, self._error = self._error, None
        if err is not None:
            raise err

    @property
    def pending(self) -> int:
        """jobs submitted and not yet written"""
        with self._cv:
            return self._submitted - self._completed

    def poll(self) -> None:
        """never blocks"""
        self._settle()

    def wait(self, ticket: int) -> None:
        """blocks until the worker is through with the job of this ticket"""
        with self._cv:
            while self._completed < ticket:
                self._cv.wait()
        self._settle()

    def finish(self) -> None:
        """every job written, the worker joined; may be called again (and `submit` starts a new worker)"""
        with self._cv:
            th, self._thread = self._thread, None
            self._stop = True
            self._cv.notify_all()
        if th is not None:
            th.join()
        self._settle()
