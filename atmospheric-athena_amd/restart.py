"""Reader / writer of the reference's restart dumps (`out_fmt = rst`, src/restart.c), the only
full-precision output format of the reference (bin and vtk are single precision).

Layout (restart.c:463-983, read back by restart_grids :52-456): the parameter dump as text,
terminated by a line ``<par_end>``; then ``N_STEP\\n`` + int32, ``\\nTIME\\n`` + double,
``\\nTIME_STEP\\n`` + double; then for every Grid the labelled blocks ``\\nDENSITY\\n``,
``\\n1-MOMENTUM\\n``, ``\\n2-MOMENTUM\\n``, ``\\n3-MOMENTUM\\n``, ``\\nENERGY\\n`` (Nx1*Nx2*Nx3 doubles
each over ACTIVE zones, [k][j][i]), with ion radiation ``\\nEDGEFLUX\\n`` ((Nx1+1)(Nx2+1)(Nx3+1)
doubles), then ``\\nSCALAR n\\n`` per passive scalar; finally ``\\nUSER_DATA\\n`` followed by whatever
the problem file writes (nothing for ifront / ioniz_sphere / blast).  With static mesh refinement
the Grid blocks of all Domains follow each other, root first (the loop over levels of
restart.c:531-770), under the one header: `write_rst_levels` / `read_rst_levels`.

With these two functions a run of this package can be continued by the reference
(``athena -r file.rst``) and vice versa, and the parity tests can start from a developed
reference state instead of the initial condition.
"""
from __future__ import annotations

import struct
from typing import Dict, Optional, Sequence

import numpy as np

from .athinput import ParTable

_LABELS = ("DENSITY", "1-MOMENTUM", "2-MOMENTUM", "3-MOMENTUM", "ENERGY")


def par_dump(par: ParTable) -> str:
    """par_dump(2, fp) of the reference (par.c:370-410): blocks, aligned `name = value` lines."""
    out = []
    for block, items in par.blocks.items():
        out.append(f"<{block}>")
        width = max((len(k) for k in items), default=0)
        for k, v in items.items():
            out.append(f"{k:<{width}} = {v}")
        out.append("")
    out.append("<par_end>")
    return "\n".join(out) + "\n"


def write_rst(path: str, par_text: str, nstep: int, time: float, dt: float, U: np.ndarray,
              edgeflux: Optional[np.ndarray] = None) -> None:
    """U: active zones [Nx3][Nx2][Nx1][nvar] (nvar = 5 or 6)."""
    if not par_text.rstrip().endswith("<par_end>"):
        par_text = par_text.rstrip("\n") + "\n<par_end>\n"
    nvar = U.shape[-1]
    with open(path, "wb") as f:
        f.write(par_text.encode())
        f.write(b"N_STEP\n" + struct.pack("<i", int(nstep)))
        f.write(b"\nTIME\n" + struct.pack("<d", float(time)))
        f.write(b"\nTIME_STEP\n" + struct.pack("<d", float(dt)))
        for c, lab in enumerate(_LABELS):
            f.write(b"\n" + lab.encode() + b"\n")
            f.write(np.ascontiguousarray(U[..., c], dtype="<f8").tobytes())
        if edgeflux is not None:
            f.write(b"\nEDGEFLUX\n")
            f.write(np.ascontiguousarray(edgeflux, dtype="<f8").tobytes())
        for n in range(nvar - 5):
            f.write(f"\nSCALAR {n}\n".encode())
            f.write(np.ascontiguousarray(U[..., 5 + n], dtype="<f8").tobytes())
        f.write(b"\nUSER_DATA\n")


def read_rst(path: str, nx: Sequence[int], nscal: int, ion: bool) -> Dict:
    b = open(path, "rb").read()
    end = b.index(b"<par_end>")
    end = b.index(b"\n", end) + 1
    header = b[:end].decode(errors="replace")
    pos = end
    if b[pos:pos + 7] != b"N_STEP\n":
        raise ValueError("[restart_grids]: Expected N_STEP")
    pos += 7
    nstep = struct.unpack_from("<i", b, pos)[0]; pos += 4

    def expect(label: bytes):
        nonlocal pos
        tag = b"\n" + label + b"\n"
        if b[pos:pos + len(tag)] != tag:
            raise ValueError(f"[restart_grids]: Expected {label.decode()}, found {b[pos:pos + 24]!r}")
        pos += len(tag)

    expect(b"TIME"); time = struct.unpack_from("<d", b, pos)[0]; pos += 8
    expect(b"TIME_STEP"); dt = struct.unpack_from("<d", b, pos)[0]; pos += 8
    n = int(nx[0]) * int(nx[1]) * int(nx[2])
    U = np.zeros((nx[2], nx[1], nx[0], 5 + nscal))
    for c, lab in enumerate(_LABELS):
        expect(lab.encode())
        U[..., c] = np.frombuffer(b, dtype="<f8", count=n, offset=pos).reshape(nx[2], nx[1], nx[0]); pos += 8 * n
    ef = None
    if ion:
        expect(b"EDGEFLUX")
        ne = (nx[0] + 1) * (nx[1] + 1) * (nx[2] + 1)
        ef = np.frombuffer(b, dtype="<f8", count=ne, offset=pos).reshape(nx[2] + 1, nx[1] + 1, nx[0] + 1).copy(); pos += 8 * ne
    for s in range(nscal):
        expect(f"SCALAR {s}".encode())
        U[..., 5 + s] = np.frombuffer(b, dtype="<f8", count=n, offset=pos).reshape(nx[2], nx[1], nx[0]); pos += 8 * n
    expect(b"USER_DATA")
    return dict(header=header, par=ParTable.from_text(header), nstep=nstep, time=time, dt=dt, U=U, edgeflux=ef)


def write_rst_levels(path: str, par_text: str, nstep: int, time: float, dt: float,
                     levels: Sequence[Sequence[Optional[np.ndarray]]]) -> None:
    """levels: [(U_active, edgeflux or None), ...] root first."""
    if not par_text.rstrip().endswith("<par_end>"):
        par_text = par_text.rstrip("\n") + "\n<par_end>\n"
    with open(path, "wb") as f:
        f.write(par_text.encode())
        f.write(b"N_STEP\n" + struct.pack("<i", int(nstep)))
        f.write(b"\nTIME\n" + struct.pack("<d", float(time)))
        f.write(b"\nTIME_STEP\n" + struct.pack("<d", float(dt)))
        for U, edgeflux in levels:
            for c, lab in enumerate(_LABELS):
                f.write(b"\n" + lab.encode() + b"\n")
                f.write(np.ascontiguousarray(U[..., c], dtype="<f8").tobytes())
            if edgeflux is not None:
                f.write(b"\nEDGEFLUX\n")
                f.write(np.ascontiguousarray(edgeflux, dtype="<f8").tobytes())
            for n in range(U.shape[-1] - 5):
                f.write(f"\nSCALAR {n}\n".encode())
                f.write(np.ascontiguousarray(U[..., 5 + n], dtype="<f8").tobytes())
        f.write(b"\nUSER_DATA\n")


def read_rst_levels(path: str, nxs: Sequence[Sequence[int]], nscal: int, ion: bool) -> Dict:
    """nxs: active zones (Nx1, Nx2, Nx3) of every level, root first."""
    b = open(path, "rb").read()
    end = b.index(b"<par_end>")
    end = b.index(b"\n", end) + 1
    header = b[:end].decode(errors="replace")
    pos = end

    def expect(label: bytes):
        nonlocal pos
        tag = (b"" if label == b"N_STEP" else b"\n") + label + b"\n"
        if b[pos:pos + len(tag)] != tag:
            raise ValueError(f"[restart_grids]: Expected {label.decode()}, found {b[pos:pos + 24]!r}")
        pos += len(tag)

    expect(b"N_STEP"); nstep = struct.unpack_from("<i", b, pos)[0]; pos += 4
    expect(b"TIME"); time = struct.unpack_from("<d", b, pos)[0]; pos += 8
    expect(b"TIME_STEP"); dt = struct.unpack_from("<d", b, pos)[0]; pos += 8
    levels = []
    for nx in nxs:
        n = int(nx[0]) * int(nx[1]) * int(nx[2])
        U = np.zeros((nx[2], nx[1], nx[0], 5 + nscal)); ef = None
        for c, lab in enumerate(_LABELS):
            expect(lab.encode())
            U[..., c] = np.frombuffer(b, dtype="<f8", count=n, offset=pos).reshape(nx[2], nx[1], nx[0]); pos += 8 * n
        if ion:
            expect(b"EDGEFLUX")
            ne = (nx[0] + 1) * (nx[1] + 1) * (nx[2] + 1)
            ef = np.frombuffer(b, dtype="<f8", count=ne, offset=pos).reshape(nx[2] + 1, nx[1] + 1, nx[0] + 1).copy(); pos += 8 * ne
        for sc in range(nscal):
            expect(f"SCALAR {sc}".encode())
            U[..., 5 + sc] = np.frombuffer(b, dtype="<f8", count=n, offset=pos).reshape(nx[2], nx[1], nx[0]); pos += 8 * n
        levels.append((U, ef))
    expect(b"USER_DATA")
    return dict(header=header, par=ParTable.from_text(header), nstep=nstep, time=time, dt=dt, levels=levels)


# ---- continuing a run (main.c -r): a reader that does not slurp the file, and the writer's pieces ------------------------------

class RestartError(ValueError):
    """ath_error of restart_grids (restart.c:52-456)"""


def section_table(nx: Sequence[int], nscal: int, ion: bool):
    """[(label, doubles)] of one Grid's sections in file order"""
    n = int(nx[0]) * int(nx[1]) * int(nx[2])
    out = [(lab, n) for lab in _LABELS]
    if ion:
        out.append(("EDGEFLUX", (int(nx[0]) + 1) * (int(nx[1]) + 1) * (int(nx[2]) + 1)))
    out += [(f"SCALAR {s}", n) for s in range(nscal)]
    return out


def expect_label(f, label: str, first: bool = False) -> None:
    """The label the reference's reader insists on at this place of the file (restart.c:79-84 ...)"""
    tag = (b"" if first else b"\n") + label.encode() + b"\n"
    got = f.read(len(tag))
    if got != tag:
        raise RestartError(f"[restart_grids]: Expected {label}, found {got!r}")


def write_header(f, par_text: str, nstep: int, time: float, dt: float) -> None:
    """Everything in front of the first Grid's sections: the parameter dump, N_STEP, TIME, TIME_STEP"""
    if not par_text.rstrip().endswith("<par_end>"):
        par_text = par_text.rstrip("\n") + "\n<par_end>\n"
    f.write(par_text.encode())
    f.write(b"N_STEP\n" + struct.pack("<i", int(nstep)))
    f.write(b"\nTIME\n" + struct.pack("<d", float(time)))
    f.write(b"\nTIME_STEP\n" + struct.pack("<d", float(dt)))


def write_grid_sections(f, U: np.ndarray, edgeflux: Optional[np.ndarray] = None) -> None:
    """One Grid's labelled sections from a host block of ACTIVE zones [Nx3][Nx2][Nx1][nvar] (engines without a device); the
    bytes lib.Grid.write_rst_payload writes for the same state."""
    for c, lab in enumerate(_LABELS):
        f.write(b"\n" + lab.encode() + b"\n")
        f.write(np.ascontiguousarray(U[..., c], dtype="<f8").tobytes())
    if edgeflux is not None:
        f.write(b"\nEDGEFLUX\n")
        f.write(np.ascontiguousarray(edgeflux, dtype="<f8").tobytes())
    for n in range(U.shape[-1] - 5):
        f.write(f"\nSCALAR {n}\n".encode())
        f.write(np.ascontiguousarray(U[..., 5 + n], dtype="<f8").tobytes())


def write_trailer(f) -> None:
    f.write(b"\nUSER_DATA\n")


def read_head(path: str) -> Dict:
    """The parameter dump (text, and parsed: comments and every block it holds), nstep / time / dt, and `offset`: where the
    first Grid's first label begins.  Reads the head of the file only."""
    import os
    with open(path, "rb") as f:
        buf = b""
        while True:
            end = buf.find(b"<par_end>")
            if end >= 0:
                nl = buf.find(b"\n", end)
                if nl >= 0:
                    break
            more = f.read(1 << 16)
            if not more:
                raise RestartError("[restart_grids]: Expected <par_end>, found the end of the file")
            buf += more
        pos = nl + 1
        header = buf[:pos].decode(errors="replace")
        f.seek(pos)
        expect_label(f, "N_STEP", first=True)
        raw = f.read(4)
        expect_label(f, "TIME"); raw += f.read(8)
        expect_label(f, "TIME_STEP"); raw += f.read(8)
        if len(raw) != 20:
            raise RestartError("[restart_grids]: Expected TIME_STEP, found the end of the file")
        nstep, time, dt = struct.unpack("<idd", raw)
        offset = f.tell()
    return dict(path=path, header=header, par=ParTable.from_text(header), nstep=nstep, time=time, dt=dt, offset=offset,
                size=os.path.getsize(path))


def index_sections(head: Dict, nxs: Sequence[Sequence[int]], nscal: int, ion: bool):
    """[[(label, byte offset of the data, doubles), ...] per level, root first] of the file behind `head` for Grids of `nxs`
    active zones.  Every label is looked at in its place and the total size must be the file's: a file of another mesh or another
    number of ranks, a truncated one, or one with bytes after USER_DATA (none of the built problems writes any) is refused."""
    levels = []
    with open(head["path"], "rb") as f:
        pos = head["offset"]
        for nx in nxs:
            secs = []
            for label, n in section_table(nx, nscal, ion):
                f.seek(pos)
                expect_label(f, label)
                pos = f.tell()
                secs.append((label, pos, n))
                pos += 8 * n
            levels.append(secs)
        f.seek(pos)
        expect_label(f, "USER_DATA")
        pos = f.tell()
    if pos != head["size"]:
        raise RestartError(f"[restart_grids]: Expected {pos} bytes, found {head['size']}")
    return levels


def scan_rst(path: str, nxs: Sequence[Sequence[int]], nscal: int, ion: bool) -> Dict:
    """read_head + index_sections"""
    head = read_head(path)
    head["levels"] = index_sections(head, nxs, nscal, ion)
    return head


def read_section(path: str, offset: int, n: int) -> np.ndarray:
    a = np.fromfile(path, dtype="<f8", count=n, offset=offset)
    if a.size != n:
        raise RestartError(f"[restart_grids]: Expected {n} doubles at byte {offset}, found {a.size}")
    return a


def read_state(head: Dict, level: int, nx: Sequence[int], nscal: int):
    """(U_active [Nx3][Nx2][Nx1][5 + nscal], edgeflux or None) of one level of an indexed file: for engines that keep a host block"""
    U = np.zeros((nx[2], nx[1], nx[0], 5 + nscal)); ef = None
    for label, off, n in head["levels"][level]:
        a = read_section(head["path"], off, n)
        if label == "EDGEFLUX":
            ef = a.reshape(nx[2] + 1, nx[1] + 1, nx[0] + 1)
        else:
            c = _LABELS.index(label) if label in _LABELS else 5 + int(label.split()[1])
            U[..., c] = a.reshape(nx[2], nx[1], nx[0])
    return U, ef


def rank_path(path0: str, rank: int) -> str:
    """The file rank r > 0 reads, from rank 0's path (main.c:265-288): ``-id<r>`` goes in front of ``.NNNN.rst``, in the same
    directory; if that does not exist, ``../id<r>/`` -- where every rank of a run wrote its own."""
    import os
    if rank == 0:
        return path0
    d, name = os.path.split(path0)
    parts = name.rsplit(".", 2)
    if len(parts) != 3:
        raise RestartError(f"[main]: restart file name {name} is not <basename>.NNNN.rst")
    sib = f"{parts[0]}-id{rank}.{parts[1]}.{parts[2]}"
    here = os.path.join(d, sib)
    if os.path.exists(here):
        return here
    there = os.path.join(d, os.pardir, f"id{rank}", sib)
    if os.path.exists(there):
        return os.path.normpath(there)
    raise RestartError(f"[main]: rank {rank} finds neither {here} nor {there}")
