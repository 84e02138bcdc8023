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
restart.c:531-770), under the one header.

One writer: `write_header`, `write_grid_sections` per Grid (or the engine's own payload from the
device, lib.Grid.write_rst_payload, between the same two), `write_trailer`.  `write_rst_levels` is
those three on a file of its own, `write_rst` its one-level case.

One reader, which never holds more than one section of the file: `read_head` (the parameter dump,
nstep, time, dt), `index_sections` (every label looked at in its place, the total size checked
against the file's) and `read_state` (one level's host block); `scan_rst` is the first two,
`read_rst_levels` all three for every level, `read_rst` its one-level case.  A file that is not
exactly the head, the sections of the Grids asked for and ``USER_DATA`` is refused with the
reference's ``[restart_grids]: Expected LABEL`` (RestartError, a ValueError) -- a truncated file,
one of another mesh, and also one with bytes after ``USER_DATA``: none of the built problems
writes any, so there is nothing they could be read into.

After that: the files of the other ranks of a run (`rank_path`), and resuming on another
decomposition (`grid_boxes`, `scan_sources`, `box_pieces`, `read_box`, `read_state_boxes`,
`regrid_par`); for a refined mesh the same per Domain (`mesh_grid_boxes`, `scan_mesh_sources`,
`regrid_mesh_par`): every Domain cut by its own NGrid_x*, the Grids dealt to the ranks in one
running count.

With this a run of this package can be continued by the reference (``athena -r file.rst``) and
vice versa, and the parity tests can start from a developed reference state instead of the
initial condition.
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


# ---- the writer: header, one Grid's sections per Grid, trailer -----------------------------------------------------------------

def _tag(label: str, first: bool = False) -> bytes:
    """A label as it stands in the file: on a line of its own, the newline in front of it closing the data before it"""
    return (b"" if first else b"\n") + label.encode() + b"\n"


def write_header(f, par_text: str, nstep: int, time: float, dt: float) -> None:
    """Everything in front of the first Grid's sections: the parameter dump, N_STEP, TIME, TIME_STEP"""
    if not par_text.rstrip().endswith("<par_end>"):
        par_text = par_text.rstrip("\n") + "\n<par_end>\n"
    f.write(par_text.encode())
    f.write(_tag("N_STEP", first=True) + struct.pack("<i", int(nstep)))
    f.write(_tag("TIME") + struct.pack("<d", float(time)))
    f.write(_tag("TIME_STEP") + struct.pack("<d", float(dt)))


def write_grid_sections(f, U: np.ndarray, edgeflux: Optional[np.ndarray] = None) -> None:
    """One Grid's labelled sections from a host block of ACTIVE zones [Nx3][Nx2][Nx1][nvar] (nvar = 5 + passive scalars; engines
    without a device); the bytes lib.Grid.write_rst_payload writes for the same state."""
    sections = [(lab, U[..., c]) for c, lab in enumerate(_LABELS)]
    if edgeflux is not None:
        sections.append(("EDGEFLUX", edgeflux))
    sections += [(f"SCALAR {n}", U[..., 5 + n]) for n in range(U.shape[-1] - 5)]
    for label, a in sections:
        f.write(_tag(label))
        f.write(np.ascontiguousarray(a, dtype="<f8").tobytes())


def write_trailer(f) -> None:
    f.write(_tag("USER_DATA"))


def write_rst_levels(path: str, par_text: str, nstep: int, time: float, dt: float,
                     levels: Sequence[Sequence[Optional[np.ndarray]]]) -> None:
    """levels: [(U_active, edgeflux or None), ...] root first."""
    with open(path, "wb") as f:
        write_header(f, par_text, nstep, time, dt)
        for U, edgeflux in levels:
            write_grid_sections(f, U, edgeflux)
        write_trailer(f)


def write_rst(path: str, par_text: str, nstep: int, time: float, dt: float, U: np.ndarray,
              edgeflux: Optional[np.ndarray] = None) -> None:
    """U: active zones [Nx3][Nx2][Nx1][nvar] (nvar = 5 or 6)."""
    write_rst_levels(path, par_text, nstep, time, dt, [(U, edgeflux)])


# ---- the reader: the head, the index of the sections, one level's state; it does not slurp the file ---------------------------

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
    tag = _tag(label, first)
    got = f.read(len(tag))
    if got != tag:
        raise RestartError(f"[restart_grids]: Expected {label}, found {got!r}")


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


def read_rst_levels(path: str, nxs: Sequence[Sequence[int]], nscal: int, ion: bool) -> Dict:
    """The whole file on the host.  nxs: active zones (Nx1, Nx2, Nx3) of every level, root first."""
    head = scan_rst(path, nxs, nscal, ion)
    levels = [read_state(head, l, nx, nscal) for l, nx in enumerate(nxs)]
    return dict(header=head["header"], par=head["par"], nstep=head["nstep"], time=head["time"], dt=head["dt"], levels=levels)


def read_rst(path: str, nx: Sequence[int], nscal: int, ion: bool) -> Dict:
    """read_rst_levels of a one-level file, the level unpacked into `U` and `edgeflux`"""
    r = read_rst_levels(path, [nx], nscal, ion)
    r["U"], r["edgeflux"] = r.pop("levels")[0]
    return r


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


# ---- resuming on another decomposition: the Grids of the run that wrote the files, and boxes out of them ------------------------

def grid_boxes(Nx: Sequence[int], ngrid: Sequence[int]):
    """[(rank, disp(3), nx(3))] of the Grids the reference cuts a root Domain of `Nx` zones into for `<domain1> NGrid_x1/2/3`
    (init_mesh.c:575-653): Nx/NGrid zones per Grid, the WHOLE remainder of a direction on the first Grid of that direction
    (:596-621), displacements accumulated (:625-653), rank ids with the x1 index fastest, then x2, then x3 (:585-591)."""
    sizes, disps = [], []
    for d in range(3):
        n, g = int(Nx[d]), int(ngrid[d])
        if g < 1:
            raise RestartError(f"[init_mesh] Cannot enter NGrid_x{d + 1}={g} in domain1")
        if g > 1 and n <= 1:
            raise RestartError(f"[init_mesh]: domain1/NGrid_x{d + 1} = {g} and Nx{d + 1} = {n}")
        q, r = divmod(n, g)
        sz = [q + r] + [q] * (g - 1)
        dp = [0]
        for v in sz[:-1]:
            dp.append(dp[-1] + v)
        sizes.append(sz); disps.append(dp)
    out = []
    for n3 in range(int(ngrid[2])):
        for m in range(int(ngrid[1])):
            for l in range(int(ngrid[0])):
                out.append((len(out), (disps[0][l], disps[1][m], disps[2][n3]), (sizes[0][l], sizes[1][m], sizes[2][n3])))
    return out


def par_ngrid(par: ParTable):
    """`<domain1> NGrid_x1/2/3` of a parameter dump, default 1 (a run started with AutoWithNProc has them written into the
    table, init_mesh.c:545-547)"""
    return tuple(par.geti("domain1", f"NGrid_x{d}") if par.exist("domain1", f"NGrid_x{d}") else 1 for d in (1, 2, 3))


def scan_sources(path0: str, rootNx: Sequence[int], nscal: int, ion: bool, head0: Optional[Dict] = None):
    """The files of the run that wrote `path0` (rank 0's file), whatever its cuts: [head with `rank`, `disp`, `nx`, `ngrid` and the
    indexed sections `levels`] in rank order.  Single-level meshes only; the number of files found through rank_path must be
    the product of the file's own NGrid_x*, and every file must have exactly the size of its box."""
    head0 = head0 or read_head(path0)
    par = head0["par"]
    nd = par.geti("job", "num_domains") if par.exist("job", "num_domains") else 1
    if nd > 1:
        raise RestartError(f"[restart_grids]: <job> num_domains = {nd}: a file of a refined mesh cannot be resumed on other cuts "
                           "(regrid takes single-level meshes only; MeshRun / MeshDriver.from_restart(regrid=True) take it)")
    ngrid = par_ngrid(par)
    boxes = grid_boxes(rootNx, ngrid)
    out = []
    for rank, disp, nx in boxes:
        try:
            p = rank_path(path0, rank)
        except RestartError:
            raise RestartError(f"[restart_grids]: Expected {len(boxes)} files for NGrid = {ngrid[0]} x {ngrid[1]} x {ngrid[2]}, "
                               f"found {rank}") from None
        head = head0 if rank == 0 else read_head(p)
        head["levels"] = index_sections(head, [nx], nscal, ion)
        head.update(rank=rank, disp=disp, nx=nx, ngrid=ngrid)
        out.append(head)
    try:
        extra = rank_path(path0, len(boxes))
    except RestartError:
        extra = None
    if extra is not None:
        raise RestartError(f"[restart_grids]: Expected {len(boxes)} files for NGrid = {ngrid[0]} x {ngrid[1]} x {ngrid[2]}, "
                           f"found {extra} as well")
    return out


def box_pieces(sources, Nx: Sequence[int], lo: Sequence[int], n: Sequence[int], edgeflux: bool = False):
    """The parts of the box [lo, lo + n) -- indices of the Domain of `Nx` zones the sources cut (the root Domain, or one Domain of
    scan_mesh_sources with its Domain-relative displacements): zones, or faces for EDGEFLUX -- that every source file holds:
    [(source, lo in the source's section, lo in the box, extent)].  Neighbouring Grids share one face index of EDGEFLUX: the
    entry comes from the upper Grid (its index 0; along x1 that is the Grid the flux enters), and the last face of a direction
    from the last Grid of that direction of the Domain."""
    out = []
    for src in sources:
        slo, dlo, ext = [], [], []
        for d in range(3):
            a = src["disp"][d]
            b = a + src["nx"][d]
            if edgeflux and b == int(Nx[d]):
                b += 1
            x0, x1 = max(a, int(lo[d])), min(b, int(lo[d]) + int(n[d]))
            if x1 <= x0:
                break
            slo.append(x0 - a); dlo.append(x0 - int(lo[d])); ext.append(x1 - x0)
        else:
            out.append((src, tuple(slo), tuple(dlo), tuple(ext)))
    return out


def read_box(src: Dict, s: int, slo: Sequence[int], ext: Sequence[int]) -> np.ndarray:
    """[ext3][ext2][ext1] doubles of section `s` of the source's Grid (entry `src["entry"]` of its indexed file, 0 where a file
    holds one Grid), from `slo` in the section's own index space: only the pages of the rows that meet the box are read."""
    label, off, cnt = src["levels"][src.get("entry", 0)][s]
    e = 1 if label == "EDGEFLUX" else 0
    nx = src["nx"]
    m = np.memmap(src["path"], dtype="<f8", mode="r", offset=off, shape=(nx[2] + e, nx[1] + e, nx[0] + e))
    a = np.ascontiguousarray(m[slo[2]:slo[2] + ext[2], slo[1]:slo[1] + ext[1], slo[0]:slo[0] + ext[0]], dtype=np.float64)
    del m
    return a


def read_state_boxes(sources, Nx: Sequence[int], lo: Sequence[int], n: Sequence[int], nscal: int):
    """(U_active [n3][n2][n1][5 + nscal], edgeflux [n3+1][n2+1][n1+1] or None) of the Grid [lo, lo + n) of the Domain of `Nx`
    zones, joined from the files of `scan_sources` (the root Domain) or one Domain's list of `scan_mesh_sources`: for engines
    that keep a host block (load_state)."""
    U = np.zeros((n[2], n[1], n[0], 5 + nscal)); ef = None
    for s, (label, _off, _cnt) in enumerate(sources[0]["levels"][sources[0].get("entry", 0)]):
        e = label == "EDGEFLUX"
        if e:
            ef = np.zeros((n[2] + 1, n[1] + 1, n[0] + 1)); dst = ef
        else:
            dst = U[..., _LABELS.index(label) if label in _LABELS else 5 + int(label.split()[1])]
        for src, slo, dlo, ext in box_pieces(sources, Nx, lo, [v + (1 if e else 0) for v in n], e):
            dst[dlo[2]:dlo[2] + ext[2], dlo[1]:dlo[1] + ext[1], dlo[0]:dlo[0] + ext[0]] = read_box(src, s, slo, ext)
    return U, ef


def regrid_par(par: ParTable, ngrid: Sequence[int], rank: int = 0, basename: Optional[str] = None) -> ParTable:
    """A copy of the table that describes a Grid of the cuts `ngrid`: NGrid_x* set, no AutoWithNProc, and for rank r > 0
    ``<job> problem_id`` with ``-id<r>`` (main.c:227-232)."""
    import copy
    q = copy.deepcopy(par)
    dom = q.blocks.setdefault("domain1", {})
    dom.pop("AutoWithNProc", None)
    for d in range(3):
        dom[f"NGrid_x{d + 1}"] = "%d" % int(ngrid[d])
    if basename is not None:
        q.blocks["job"]["problem_id"] = basename + ("-id%d" % rank if rank else "")
    return q


# ---- the same for a refined mesh: every Domain cut by its own NGrid_x*, the Grids dealt to the ranks in one running count --------

def domain_blocks(par: ParTable):
    """The N of every <domainN> in the order of the reference's loops: level by level, deck order inside a level (config.levels)"""
    nd = par.geti("job", "num_domains") if par.exist("job", "num_domains") else 1
    return [n for _lev, n in sorted(((par.geti(f"domain{n}", "level") if par.exist(f"domain{n}", "level") else 0), n)
                                    for n in range(1, nd + 1))]


def par_mesh_ngrid(par: ParTable):
    """par_ngrid of every <domainN>, in the order of domain_blocks"""
    return [tuple(par.geti(f"domain{n}", f"NGrid_x{d}") if par.exist(f"domain{n}", f"NGrid_x{d}") else 1 for d in (1, 2, 3))
            for n in domain_blocks(par)]


def mesh_nproc(ngrids, nproc: Optional[int] = None) -> int:
    """The number of ranks a mesh whose Domains are cut by `ngrids` runs on: `nproc` checked against init_mesh.c:564-567 (no
    Domain has more Grids than there are ranks) and :661 (the running count ends at 0: the ranks divide the number of Grids), or,
    without it, the smallest count that passes both.  ValueError otherwise."""
    cnt = [int(g[0]) * int(g[1]) * int(g[2]) for g in ngrids]
    if not cnt or min(cnt) < 1:
        raise ValueError(f"[init_mesh]: NGrid = {list(ngrids)!r} (three counts >= 1 per Domain)")
    total, most = sum(cnt), max(cnt)
    if nproc is None:
        return next(p for p in range(most, total + 1) if total % p == 0)
    if int(nproc) < most or total % int(nproc):
        raise ValueError(f"[init_mesh]: {total} Grids, {most} of them in one Domain, cannot be dealt to {nproc} ranks")
    return int(nproc)


def mesh_grid_boxes(domains, nproc: int):
    """Per Domain the [(rank, disp(3), nx(3))] of its Grids.  domains: [(Nx, NGrid)] level by level, deck order inside a level.
    Every Domain is cut like the root (grid_boxes: Nx / NGrid zones, the whole remainder on the first Grid of a direction;
    `disp` is relative to the Domain, the reference adds the Domain's own Disp, init_mesh.c:625-653); the Grids take consecutive
    world ranks, x1 index fastest, and the count runs on from Domain to Domain, wrapping at `nproc` (:589-590).  It must end at
    0 (:661), and no Domain may have more Grids than there are ranks (:564-567) -- so a rank holds at most one Grid per Domain,
    and possibly none of the root."""
    nproc = int(nproc)
    out, nxt, total = [], 0, 0
    for n, (Nx, ngrid) in enumerate(domains):
        boxes = grid_boxes(Nx, ngrid)
        if len(boxes) > nproc:
            raise RestartError(f"[restart_grids]: Expected at least {len(boxes)} files for the NGrid = {ngrid[0]} x {ngrid[1]} x "
                               f"{ngrid[2]} of Domain {n} (a Domain has no more Grids than there are ranks), found {nproc}")
        out.append([((nxt + r) % nproc, disp, nx) for r, disp, nx in boxes])
        nxt = (nxt + len(boxes)) % nproc
        total += len(boxes)
    if nxt != 0:
        raise RestartError(f"[restart_grids]: Expected a number of files that divides the {total} Grids of the mesh, found {nproc}")
    return out


def scan_mesh_sources(path0: str, domains, nscal: int, ion: bool, head0: Optional[Dict] = None):
    """scan_sources for a refined mesh.  domains: Nx of every Domain (or anything with `.Nx`: config.levels), level by level;
    their cuts are the file's own ``<domainN> NGrid_x1/2/3``.  The number of ranks is the number of files found through
    rank_path; every file is indexed for exactly the Grids its rank holds by mesh_grid_boxes, in Domain order (restart.c:531-770)
    -- a file of another size, of other cuts or of another number of ranks is refused by index_sections.
    -> per Domain [source]: the file's head with `levels` (the sections of every Grid in the file) and this Grid's `rank`,
    `disp` (relative to the Domain), `nx`, `ngrid` and `entry`, its place in `levels`."""
    head0 = head0 or read_head(path0)
    ngrids = par_mesh_ngrid(head0["par"])
    Nxs = [tuple(int(v) for v in getattr(d, "Nx", d)) for d in domains]
    if len(ngrids) != len(Nxs):
        raise RestartError(f"[restart_grids]: Expected {len(Nxs)} Domains, found <job> num_domains = {len(ngrids)}")
    paths = [path0]
    while True:
        try:
            paths.append(rank_path(path0, len(paths)))
        except RestartError:
            break
    table = mesh_grid_boxes(list(zip(Nxs, ngrids)), len(paths))
    out = [[] for _ in Nxs]
    for rank, p in enumerate(paths):
        head = head0 if rank == 0 else read_head(p)
        mine = [(n, b) for n, boxes in enumerate(table) for b in boxes if b[0] == rank]
        head["levels"] = index_sections(head, [b[2] for _n, b in mine], nscal, ion)
        for entry, (n, (_r, disp, nx)) in enumerate(mine):
            out[n].append(dict(head, rank=rank, disp=disp, nx=nx, ngrid=ngrids[n], entry=entry))
    return out


def read_section_boxes(sources, Nx: Sequence[int], s: int) -> np.ndarray:
    """Section `s` of the whole Domain of `Nx` zones joined on the host from one Domain's sources: what a handle that takes whole
    sections only (a Grid cut into slabs inside the library) is given."""
    e = 1 if sources[0]["levels"][sources[0].get("entry", 0)][s][0] == "EDGEFLUX" else 0
    dims = [int(v) + e for v in Nx]
    a = np.zeros((dims[2], dims[1], dims[0]))
    for src, slo, dlo, ext in box_pieces(sources, Nx, (0, 0, 0), dims, bool(e)):
        a[dlo[2]:dlo[2] + ext[2], dlo[1]:dlo[1] + ext[1], dlo[0]:dlo[0] + ext[0]] = read_box(src, s, slo, ext)
    return a


def regrid_mesh_par(par: ParTable, ngrids, rank: int = 0, basename: Optional[str] = None) -> ParTable:
    """regrid_par for every <domainN>: `ngrids` in the order of domain_blocks"""
    import copy
    q = copy.deepcopy(par)
    for n, ngrid in zip(domain_blocks(q), ngrids):
        dom = q.blocks.setdefault(f"domain{n}", {})
        dom.pop("AutoWithNProc", None)
        for d in range(3):
            dom[f"NGrid_x{d + 1}"] = "%d" % int(ngrid[d])
    if basename is not None:
        q.blocks["job"]["problem_id"] = basename + ("-id%d" % rank if rank else "")
    return q
