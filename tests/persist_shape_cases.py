"""Launch forms of the persistent Lanczos kernel (k_lanc_persist,
csrc/ed_persist.hpp) outside real-vector MODE 4, one table entry per form, and
the CPU side of their tests: the host's geometry formulas restated on the
oracle's CSR, and an extended-precision Lanczos reference.

Shared by tests/test_persist_shapes_cpu.py (proves the table and the
reference margins from the oracle alone) and tests/test_gpu_persist_shapes.py
(runs every entry and asserts Sector.lanc_geom, the library's own answer).
Real-vector MODE 4 has its table in tests/persist_mode4_cases.py.

A form is (mode, HC, VC, width, RPT): HC = H held as complex(8) (a Sector
built without real=True, whatever its values), VC = complex(8) vectors, width
the ELL row width W (modes 2/3), the hop-list width E (mode 4) or 1 (modes
0/1), RPT the row slots per thread.  "rr" = real H, real v; "rc" = real H,
complex v; "cc" = complex H, complex v.  "nbN" = make_config(Norb=1, Nbath=N).
Each form takes the smallest pool sector of dim >= 36 that reaches it; where
that sector has a flat Norb=1 bath (two distinct hop values) and the pool
also holds a sector with a richer dictionary or without Kronecker form, the
latter is a second entry of the same form (normal_jh, hybrid).  One sector is
passed over: nb8 (1,1), 81 rows, is the smallest with W = 16, but with eight
degenerate bath levels its recurrence is ill-conditioned: the persistent and
the multi-kernel run, which differ only in summation order, are 1.5e-5 to
2.4e-5 apart by step 40 (1e-13 from the reference at step 24), so it cannot
be held to the multi-kernel comparison; nb8 (2,1) takes its place.

How a form is forced (persist_mode_derive, csrc/ed_lanczos.hip):
  mode 0  stored sector, option persist_stored
  mode 1  matrix-free sector with Kronecker form, option no_preg
  mode 2  stored sector, option no_pkron (else a real Norb=1 H takes MODE 4)
  mode 3  matrix-free sector with Kronecker form, option no_pkron
  mode 4  real H with Kronecker form, no option; complex vectors here

Modes 2 and 3: W in {8, 12, 14, 16} x RPT in {2, 4, 6, 8, 10}, dim <= 5,120,
RPT * W <= preg_cap = 112 (rr), 84 (rc), 80 (cc).
  covered, rr  (8,2) nb3 (2,2)   (8,4) nb6 (3,3)   (8,10) nb7 (4,4)
               (12,2) nb5 (1,1) and, mode 2, normal_jh (3,3)
               (12,4) nb7 (3,2)  (12,8) nb7 (3,3)
               (14,2) nb7 (1,1)  (14,4) nb8 (4,1)  (14,6) nb9 (5,1)
               (14,8) c5 (7,0), mode 2 only (nonsu2: no Kronecker form)
               (16,2) nb8 (2,1) and, mode 2, hybrid (4,2)
               (16,4) nb9 (3,1)  (16,6) nb9 (4,1)
  covered, rc  the rr sectors of (8,2) (8,4) (8,10) (12,2) (12,4) (14,2)
               (14,4) (14,6) (16,2) (16,4)
  covered, cc  mode 2: (8,2) nonsu2_replica (3,0)   (12,2) nonsu2_replica (4,0)
               (14,2) replica_cplx (3,3)            (14,4) replica_cplx Nbath=3 (3,2)
               (16,2) nonsu2_replica Nbath=5 (6,0)  (16,4) nonsu2_replica Nbath=6 (5,0)
               mode 3: (12,2) replica_cplx (2,4)    (14,2) replica_cplx (3,3)
               (14,4) replica_cplx Nbath=3 (3,2)
               and, real values held as complex(8) (these run the HC code but
               cannot show a missing conjugate): (8,4) nb6 (3,3), (8,10) nb7
               (4,4), (12,4) nb7 (3,2) in modes 2 and 3; (8,2) nb3 (2,2),
               (16,2) nb8 (2,1), (16,4) nb9 (3,1) in mode 3
  unreachable behind the caps
               rr (12,10) (14,10) (16,8) (16,10); rc also (12,8) (12,10)
               (14,8) (16,6); cc also (12,8) (14,6) (14,8) (16,6); mode 3 cc
               above a 16 KiB dictionary (nb9 (4,1): 21.6 KB)
  not reached by the pool
               (8,6) (8,8) (12,6) in every (HC, VC) case (W = 8 needs both
               spins at half filling: nb7 (4,4) is the only Norb=1 sector
               above 2,048 rows; no pool sector has 2,049-3,072 rows and a
               longest row of 9-12); mode 3 rr (14,8) (3,073-4,096 rows with a
               longest row of 13-14: only c5 (7,0), which is nonsu2)

Modes 0 and 1: the template RPT is persist_rpt01(dim) = ceil(dim / 1024),
rounded up to 8 above 6; width 1.
  covered, rr  1 nb3 (2,2)  2 nb6 (3,3)  3 nb9 (4,1)  4 nb7 (3,3)  5 nb7 (4,4)
               6 nb9 (3,2)  8 nb8 (3,3)
  covered, rc  1-5, the same sectors
  covered, cc  mode 0: 1 nonsu2_replica (3,0)  2 replica_cplx Nbath=3 (3,2)
               4 replica_cplx Nbath=3 (3,3) (longest row 16: 16 * 8 words are
               too many for the register modes)  5 replica_cplx Nbath=3 (4,4)
               (longest row 20)
               mode 1: 1 replica_cplx (3,3), 2, 4, 5 as mode 0
               class 3, both modes: nb9 (4,1) held as complex(8) (no replica
               sector of the pool has 2,049-3,072 rows)
  unreachable behind the caps
               rr 10, 12, 16 and rc / cc 6-16: persist_mode_derive's rpt_max
               (8 rows per thread real/real, 5 otherwise) refuses the sector
               before the dispatch's RPT 10, 12 and 16 can be chosen; rr 7
               does not exist (persist_rpt01 rounds it to 8).  Not tested.

MODE 4 with complex vectors (rc; 512 threads, E = 4 with RPT <= 10, E = 8 with
RPT <= 6): the seven sectors of persist_mode4_cases.CASES, stored; nb3 (2,2)
(idle lanes) and nb7 (3,2) (E = 8) also matrix-free (diagonal generated in the
kernel).
  covered      (4,2) nb3 (2,2), nb5 (3,3)  (4,4) nb6 (3,3)  (4,10) nb7 (4,4)
               (8,2) nb7 (2,2)  (8,4) nb7 (3,2)  (8,6) nb8 (3,2)
  not reached  (4,6) (4,8)

Kronecker form of the replica baths (info.kron; the GPU test asserts it):
replica_cplx is normal mode without Jx / Jp, so its matrix-free sectors have
it (modes 1 and 3 with a complex H run); nonsu2_replica has not (its
matrix-free sectors run the multi-kernel recurrence) and appears in the stored
modes only.
"""
from collections import namedtuple
from functools import lru_cache, partial
from math import comb

import numpy as np

import cases
import persist_mode4_cases as pc
from edgpu.params import make_config

NT_REG, NT_LDS = 512, 1024          # kPRegBlock (modes 2-4), kPBlock (modes 0/1)
LDS_BUDGET = 150 * 1024             # kLdsBudget
DICT_BYTES = 1 << 14                # kPkOffMask + 1
NSTEP_REF = 24                      # steps compared with the extended-precision reference
NSTEP_MULTI = 40                    # steps compared with the multi-kernel recurrence
NPROBE_MAX = 96                     # unit-vector probes per batched launch

Shape = namedtuple("Shape", "id factory sector dim dimup kw options mode hc vc width rpt")


@lru_cache(maxsize=None)
def nb(n):
    return partial(make_config, Norb=1, Nbath=n)


def _dimup(n, nup):
    return comb(n + 1, nup)


_KW = {"rr": (True, False, False), "rc": (True, False, True), "cc": (False, True, True)}
_FORCE = {0: (True, ("persist_stored",)), 1: (False, ("no_preg",)), 2: (True, ("no_pkron",)),
          3: (False, ("no_pkron",)), 4: (True, ())}


# rows of each pool sector (tests/test_persist_shapes_cpu.py checks them against the oracle)
DIMS = {"nb3_2_2": 36, "nb5_1_1": 36, "nb5_3_3": 400, "nb6_3_3": 1225, "nb7_1_1": 64, "nb7_2_2": 784,
        "nb7_3_2": 1568, "nb7_3_3": 3136, "nb7_4_4": 4900, "nb8_2_1": 324, "nb8_3_2": 3024, "nb8_3_3": 7056,
        "nb8_4_1": 1134, "nb9_3_1": 1200, "nb9_3_2": 5400, "nb9_4_1": 2100, "nb9_5_1": 2520,
        "c5_7_0": 3432, "normal_jh_3_3": 400, "hybrid_4_2": 225,
        "nonsu2_replica_3_0": 56, "nonsu2_replica_4_0": 70, "nonsu2_replica5_6_0": 924,
        "nonsu2_replica6_5_0": 2002, "replica_cplx_2_4": 225, "replica_cplx_3_3": 400,
        "replica_cplx3_3_2": 1568, "replica_cplx3_3_3": 3136, "replica_cplx3_4_4": 4900}


def _entry(tag, factory, sector, dimup, mode, vt, width, rpt, stored=None):
    real, hc, vc = _KW[vt]
    st, opts = _FORCE[mode]
    if stored is not None:
        st = stored
    kw = dict(stored=True, real=real) if st else dict(stored=False, direct=True, real=real)
    wid = {0: "r%d" % rpt, 1: "r%d" % rpt}.get(mode, "%dx%d" % (width, rpt))
    ident = "m%d%s_%s_%s_%s" % (mode, "" if st == _FORCE[mode][0] else ("s" if st else "d"), vt, wid, tag)
    return Shape(ident, factory, sector, DIMS[tag], dimup, kw, opts, mode, hc, vc, width, rpt)


def _table():
    t = []
    rcplx3, nrep5, nrep6 = partial(cases.replica_cplx, 3), partial(cases.nonsu2_replica, 5), \
        partial(cases.nonsu2_replica, 6)
    # ---- modes 2 and 3, real H: (W, RPT, tag, factory, sector, dimup or None, rc too)
    reg = [
        (8, 2, "nb3_2_2", nb(3), (2, 2), _dimup(3, 2), True),
        (8, 4, "nb6_3_3", nb(6), (3, 3), _dimup(6, 3), True),
        (8, 10, "nb7_4_4", nb(7), (4, 4), _dimup(7, 4), True),
        (12, 2, "nb5_1_1", nb(5), (1, 1), _dimup(5, 1), True),
        (12, 2, "normal_jh_3_3", cases.normal_jh, (3, 3), None, False),
        (12, 4, "nb7_3_2", nb(7), (3, 2), _dimup(7, 3), True),
        (12, 8, "nb7_3_3", nb(7), (3, 3), _dimup(7, 3), False),
        (14, 2, "nb7_1_1", nb(7), (1, 1), _dimup(7, 1), True),
        (14, 4, "nb8_4_1", nb(8), (4, 1), _dimup(8, 4), True),
        (14, 6, "nb9_5_1", nb(9), (5, 1), _dimup(9, 5), True),
        (14, 8, "c5_7_0", cases.c5, (7, 0), None, False),
        (16, 2, "nb8_2_1", nb(8), (2, 1), _dimup(8, 2), True),
        (16, 2, "hybrid_4_2", cases.hybrid, (4, 2), None, False),
        (16, 4, "nb9_3_1", nb(9), (3, 1), _dimup(9, 3), True),
        (16, 6, "nb9_4_1", nb(9), (4, 1), _dimup(9, 4), False),
    ]
    for W, R, tag, fac, sec, du, rc in reg:
        for mode in (2, 3):
            if mode == 3 and du is None:
                continue
            t.append(_entry(tag, fac, sec, du, mode, "rr", W, R))
            if rc and du is not None:
                t.append(_entry(tag, fac, sec, du, mode, "rc", W, R))
    # ---- modes 2 and 3, complex H
    for W, R, tag, fac, sec, du, modes in [
        (8, 2, "nonsu2_replica_3_0", cases.nonsu2_replica, (3, 0), None, (2,)),
        (12, 2, "nonsu2_replica_4_0", cases.nonsu2_replica, (4, 0), None, (2,)),
        (12, 2, "replica_cplx_2_4", cases.replica_cplx, (2, 4), comb(6, 2), (3,)),
        (14, 2, "replica_cplx_3_3", cases.replica_cplx, (3, 3), comb(6, 3), (2, 3)),
        (14, 4, "replica_cplx3_3_2", rcplx3, (3, 2), comb(8, 3), (2, 3)),
        (16, 2, "nonsu2_replica5_6_0", nrep5, (6, 0), None, (2,)),
        (16, 4, "nonsu2_replica6_5_0", nrep6, (5, 0), None, (2,)),
        (8, 2, "nb3_2_2", nb(3), (2, 2), _dimup(3, 2), (3,)),
        (8, 4, "nb6_3_3", nb(6), (3, 3), _dimup(6, 3), (2, 3)),
        (8, 10, "nb7_4_4", nb(7), (4, 4), _dimup(7, 4), (2, 3)),
        (12, 4, "nb7_3_2", nb(7), (3, 2), _dimup(7, 3), (2, 3)),
        (16, 2, "nb8_2_1", nb(8), (2, 1), _dimup(8, 2), (3,)),
        (16, 4, "nb9_3_1", nb(9), (3, 1), _dimup(9, 3), (3,)),
    ]:
        for mode in modes:
            t.append(_entry(tag, fac, sec, du, mode, "cc", W, R))
    # ---- modes 0 and 1 by RPT class
    cls_real = [(1, "nb3_2_2", nb(3), (2, 2), _dimup(3, 2)), (2, "nb6_3_3", nb(6), (3, 3), _dimup(6, 3)),
                (3, "nb9_4_1", nb(9), (4, 1), _dimup(9, 4)), (4, "nb7_3_3", nb(7), (3, 3), _dimup(7, 3)),
                (5, "nb7_4_4", nb(7), (4, 4), _dimup(7, 4)), (6, "nb9_3_2", nb(9), (3, 2), _dimup(9, 3)),
                (8, "nb8_3_3", nb(8), (3, 3), _dimup(8, 3))]
    for R, tag, fac, sec, du in cls_real:
        for mode in (0, 1):
            t.append(_entry(tag, fac, sec, du, mode, "rr", 1, R))
            if R <= 5:
                t.append(_entry(tag, fac, sec, du, mode, "rc", 1, R))
    for R, tag, fac, sec, du, modes in [
        (1, "nonsu2_replica_3_0", cases.nonsu2_replica, (3, 0), None, (0,)),
        (1, "replica_cplx_3_3", cases.replica_cplx, (3, 3), comb(6, 3), (1,)),
        (2, "replica_cplx3_3_2", rcplx3, (3, 2), comb(8, 3), (0, 1)),
        (3, "nb9_4_1", nb(9), (4, 1), _dimup(9, 4), (0, 1)),
        (4, "replica_cplx3_3_3", rcplx3, (3, 3), comb(8, 3), (0, 1)),
        (5, "replica_cplx3_4_4", rcplx3, (4, 4), comb(8, 4), (0, 1)),
    ]:
        for mode in modes:
            t.append(_entry(tag, fac, sec, du, mode, "cc", 1, R))
    # ---- MODE 4, complex vectors: the sectors of persist_mode4_cases
    for c in pc.CASES:
        t.append(_entry(pc.key(c), nb(c[0]), c[1], c[2][0], 4, "rc", c[3], c[4]))
    for c in pc.CASES:
        if pc.key(c) in ("nb3_2_2", "nb7_3_2"):
            t.append(_entry(pc.key(c), nb(c[0]), c[1], c[2][0], 4, "rc", c[3], c[4], stored=False))
    return t


TABLE = _table()
IDS = [e.id for e in TABLE]
assert len(set(IDS)) == len(IDS)


def nthreads(mode):
    return NT_REG if mode >= 2 else NT_LDS


def form(e):
    return (e.mode, e.hc, e.vc, e.width, e.rpt)


def launch_entries():
    """One entry per (mode, HC, VC) for the launch-path legs, a padded one
    (dim no multiple of the workgroup, last row slot partly empty) with more
    than one row slot in use where the table has it, for a complex H one with
    complex values, the smallest such."""
    best = {}
    for e in TABLE:
        dim = e.dim
        nt = nthreads(e.mode)
        real_values = getattr(e.factory, "func", None) is make_config
        rank = (not (dim % nt != 0 and dim > nt), e.hc and real_values, dim)
        k = (e.mode, e.hc, e.vc)
        if k not in best or rank < best[k][0]:
            best[k] = (rank, e)
    return [v[1] for _, v in sorted(best.items())]


# ----------------------------------------------------------------- oracle side
@lru_cache(maxsize=4)
def _oracle_csr(ident_key):
    from oracle.oracle import Oracle

    e = next(x for x in TABLE if (x.factory, x.sector) == ident_key)
    orc = Oracle(e.factory())
    hmap = orc.build_sector(*e.sector)
    return orc.build_csr(hmap), len(hmap)


def oracle_csr(e):
    """(csr, dim) of the entry's sector from the oracle (cached: entries of one
    sector follow each other in the table)."""
    return _oracle_csr((e.factory, e.sector))


def persist_rpt01(dim):
    r = -(-dim // NT_LDS)
    return r if r <= 6 else 8 if r <= 8 else 10 if r <= 10 else 12 if r <= 12 else 16


def preg_cap(hc, vc):
    return (80 if hc else 84) if vc else 112


def _rpt_class(n):
    return next((r for r in (2, 4, 6, 8, 10) if n <= r), 0)


def _width(w):
    return next((x for x in (8, 12, 14, 16) if w <= x), 0)


def geometry_from_csr(csr, dim, hc, vc, dimup=None):
    """The numbers build_preg, pkr_geom and persist_rpt01 derive, from the
    oracle's CSR: longest off-diagonal row and its ELL width W, the register
    modes' RPT, the 1024-thread modes' RPT class, the dictionary size; with
    dimup (rows are iw * dimup + iu) also whether every off-diagonal element
    moves one spin only, the hop degrees and MODE 4's (E, RPT)."""
    rowptr, cols, vals = csr
    rows = np.repeat(np.arange(dim), np.diff(rowptr))
    off = cols != rows
    cnt = np.bincount(rows[off], minlength=dim)
    wmax = int(cnt.max())
    ov = np.ascontiguousarray(vals[off])
    bits = ov.view(np.uint64).reshape(-1, 2)
    if not hc:
        bits = bits[:, :1]
    g = dict(dim=dim, wmax=wmax, W=_width(wmax), RPT=_rpt_class(-(-dim // NT_REG)),
             rpt01=persist_rpt01(dim), rpt_max=5 if (vc or hc) else 8, cap=preg_cap(hc, vc),
             cplx=bool(np.any(vals.imag != 0.0)), diag_real=bool(np.all(vals[~off].imag == 0.0)),
             ndict=1 + len(np.unique(bits, axis=0)), kron=False)
    if dimup:
        du, dd = dimup, dim // dimup
        r, c = rows[off], cols[off].astype(np.int64)
        up = (r // du == c // du)
        dw = (r % du == c % du)
        g["kron"] = bool(du * dd == dim and np.all(up ^ dw))
        g["du"], g["dd"] = du, dd
        g["degu"] = int(np.bincount(r[up], minlength=dim).max()) if up.any() else 0
        g["degd"] = int(np.bincount(r[dw], minlength=dim).max()) if dw.any() else 0
        deg = max(g["degu"], g["degd"])
        g["E"] = 4 if deg <= 4 else 8 if deg <= 8 else 0
        G = NT_REG // du if du <= NT_REG else 0
        g["RPT4"] = _rpt_class(-(-dd // G)) if G else 0
    return g


def _al(b):
    return (b + 15) & ~15


def derive_mode(g, e):
    """persist_mode_derive's decision for the entry's path, options and vector
    type on the geometry g: (mode, width, RPT), or (-1, 0, 0)."""
    none = (-1, 0, 0)
    o = set(e.options)
    stored = e.kw.get("stored", False)
    hc, vc, dim = e.hc, e.vc, g["dim"]
    vs, hs = (16 if vc else 8), (16 if hc else 8)
    if "no_persist" in o or dim > g["rpt_max"] * NT_LDS:
        return none
    lds0 = _al(NT_LDS * g["rpt01"] * vs)
    kron = g["kron"]
    if not (o & {"no_pkron", "no_preg"}) and kron and not hc and not (stored and "persist_stored" in o):
        E, R = g["E"], g["RPT4"]
        fits = E and R and R * (3 * E + 8) + 3 * E <= 216
        fits_c = (R <= 10) if E == 4 else (R <= 6)
        if fits and (not vc or fits_c):
            vr = NT_REG * R
            lds = _al(vr * vs) + E * g["dd"] * 8 if vc else _al((vr + R) * vs)
            if lds <= LDS_BUDGET:
                return 4, E, R
    if stored:
        if "persist_stored" in o:
            return (0, 1, g["rpt01"]) if lds0 <= LDS_BUDGET else none
        if "no_preg" in o or dim > 10 * NT_REG or not g["W"] or (hc and not g["diag_real"]):
            return none
        if g["ndict"] * hs > DICT_BYTES or g["RPT"] * g["W"] > g["cap"]:
            return none
        vr = NT_REG * g["RPT"]
        if _al(vr * vs) + _al(vr * 8) + _al(g["ndict"] * hs) > LDS_BUDGET:
            return none
        return 2, g["W"], g["RPT"]
    if not kron:
        return none
    tab = g["degu"] * g["du"] + g["degd"] * g["dd"]
    if "no_preg" not in o and dim <= 10 * NT_REG:
        W = _width(g["degu"] + g["degd"])
        vr = NT_REG * g["RPT"]
        l3 = _al((tab + 1) * hs) + _al(vr * vs) + _al(vr * 8)
        if W and g["RPT"] * W <= g["cap"] and (tab + 1) * hs <= DICT_BYTES and l3 <= LDS_BUDGET and g["diag_real"]:
            return 3, W, g["RPT"]
    lds1 = lds0 + (g["du"] + g["dd"]) * (hs + 33) + tab * (hs + 4) + 16 * 16 * 8 + 256
    return (1, 1, g["rpt01"]) if lds1 <= LDS_BUDGET else none


# ------------------------------------------------------------------ reference
def ell_from_csr(csr, dim):
    """The CSR as padded (dim, width) column / value arrays in row order
    (padding: column 0, value 0)."""
    rowptr, cols, vals = csr
    cnt = np.diff(rowptr)
    C = np.zeros((dim, int(cnt.max())), dtype=np.int64)
    A = np.zeros((dim, int(cnt.max())), dtype=np.complex128)
    rows = np.repeat(np.arange(dim), cnt)
    k = np.arange(len(cols)) - np.repeat(rowptr[:-1], cnt)
    C[rows, k] = cols
    A[rows, k] = vals
    return C, A


def lanczos_columns(ell, V0, nitermax, threshold=1e-13, dtype=np.clongdouble, reverse=False):
    """orc_lanc_tridiag (oracle/ed_oracle.c) line for line in `dtype`, for every
    column of V0 (dim, k) at once: (alfa (k, nitermax), beta (k, nitermax),
    steps done (k,)).  Rows of H are summed in stored order, or last entry
    first with reverse.  dtype clongdouble is the extended-precision reference
    (64-bit mantissa: eps 1.1e-19)."""
    C, A = ell
    A = A.astype(dtype)
    rdt = np.zeros(1, dtype=dtype).real.dtype
    vin = np.array(V0, dtype=dtype, copy=True)
    if vin.ndim == 1:
        vin = vin[:, None]
    dim, k = vin.shape
    vout = np.zeros_like(vin)
    alfa = np.zeros((k, nitermax), dtype=rdt)
    beta = np.zeros((k, nitermax), dtype=rdt)
    done = np.zeros(k, dtype=np.int64)
    live = np.ones(k, dtype=bool)
    b = np.zeros(k, dtype=rdt)
    order = range(C.shape[1] - 1, -1, -1) if reverse else range(C.shape[1])

    def dot(x, y):
        return np.sum(x.real * y.real + x.imag * y.imag, axis=0)

    with np.errstate(divide="ignore", invalid="ignore"):
        for it in range(1, nitermax + 1):
            if it == 1:
                vin = vin / np.sqrt(dot(vin, vin))
                b[:] = 0
            tmp = np.zeros_like(vin)
            for q in order:
                tmp = tmp + A[:, q, None] * vin[C[:, q]]
            tmp = tmp - b * vout
            a = dot(vin, tmp)
            tmp = tmp - a * vin
            b = np.sqrt(dot(tmp, tmp))
            vout = vin
            vin = tmp / b
            alfa[live, it - 1] = a[live]
            if it < nitermax:
                beta[live, it] = b[live]
            done[live] = it
            live = live & ~(np.abs(b) < threshold)
            if not live.any():
                break
    return alfa, beta, done


def start(e, dim):
    """Start vector of leg A: the oracle's start_vector, its real part for
    real vectors."""
    from oracle.oracle import start_vector

    v = start_vector(dim)
    return v if e.vc else np.ascontiguousarray(v.real)


def window(dim):
    return min(NSTEP_REF, dim // 2)


def probe_columns(e, dim):
    """Columns j of the unit-vector probes e_j: the ends, both sides of every
    workgroup-sized row slot boundary, the first column of every DimUp block
    (MODE 4 complex: the row slots follow the down index there) and 32 more at
    a fixed stride.  The GPU test runs them NPROBE_MAX seeds to a launch."""
    nt = nthreads(e.mode)
    cols = [0, dim - 1]
    for k in range(1, -(-dim // nt) + 1):
        cols += [k * nt - 1, k * nt, k * nt + 1]
    if e.mode == 4:
        cols += [g * e.dimup for g in range(dim // e.dimup)]
    cols += [(7 + j * max(1, dim // 32)) % dim for j in range(32)]
    return np.array(sorted({j for j in cols if 0 <= j < dim}), dtype=np.int64)


def hnorm_inf(csr, dim):
    rowptr, cols, vals = csr
    rows = np.repeat(np.arange(dim), np.diff(rowptr))
    return float(np.bincount(rows, weights=np.abs(vals), minlength=dim).max())


def column_facts(csr, dim, cols_j):
    """Per probed column j: H_jj as the oracle stores it and the 2-norm of the
    column's off-diagonal part (extended precision).  H is Hermitian, so the
    column's entries are the conjugates of row j's."""
    rowptr, cols, vals = csr
    hjj = np.zeros(len(cols_j))
    nrm = np.zeros(len(cols_j), dtype=np.longdouble)
    for n, j in enumerate(cols_j):
        sl = slice(rowptr[j], rowptr[j + 1])
        c, v = cols[sl], vals[sl]
        d = v[c == j]
        hjj[n] = d[0].real if len(d) else 0.0
        o = v[c != j]
        nrm[n] = np.sqrt(np.sum(o.real.astype(np.longdouble) ** 2 + o.imag.astype(np.longdouble) ** 2))
    return hjj, nrm


# ------------------------------------------------- references, once per sector
NPROBE_STEPS = 3   # alpha[0..1] and beta[1..2] are two full steps; beta[2] needs a third slot


@lru_cache(maxsize=None)
def _reference_run(key, vc):
    from oracle.oracle import lanc_tridiag

    e = next(x for x in TABLE if (x.factory, x.sector) == key and x.vc == vc)
    csr, dim = oracle_csr(e)
    ell = ell_from_csr(csr, dim)
    n = min(NSTEP_MULTI, dim // 2)
    v0 = start(e, dim)
    ext = lanczos_columns(ell, v0, n)
    rev = lanczos_columns(ell, v0, n, dtype=np.complex128, reverse=True)
    return dict(n=n, m=window(dim), v0=v0, oracle=lanc_tridiag(csr, v0, n),
                ext=(ext[0][0], ext[1][0], int(ext[2][0])), rev=(rev[0][0], rev[1][0], int(rev[2][0])))


def reference_run(e):
    """Leg A's runs of min(40, dim // 2) steps from start(e, dim): the oracle's
    (f64), the extended-precision one (longdouble arrays) and the f64 one that
    sums each row last entry first; m = the window compared with the GPU."""
    return _reference_run((e.factory, e.sector), e.vc)


@lru_cache(maxsize=None)
def _reference_probes(key, mode, dimup):
    from oracle.oracle import lanc_tridiag

    e = next(x for x in TABLE if (x.factory, x.sector) == key and nthreads(x.mode) == nthreads(mode)
             and (x.mode == 4) == (mode == 4))
    csr, dim = oracle_csr(e)
    ell = ell_from_csr(csr, dim)
    cols = probe_columns(e, dim)
    k = len(cols)
    seeds = np.zeros((dim, k))
    seeds[cols, np.arange(k)] = 1.0
    ext = lanczos_columns(ell, seeds, NPROBE_STEPS)
    ao, bo, no = np.zeros((k, NPROBE_STEPS)), np.zeros((k, NPROBE_STEPS)), np.zeros(k, dtype=np.int64)
    for q in range(k):
        ao[q], bo[q], no[q] = lanc_tridiag(csr, seeds[:, q], NPROBE_STEPS)
    hjj, cnorm = column_facts(csr, dim, cols)
    return dict(cols=cols, ext=ext, oracle=(ao, bo, no), hjj=hjj, cnorm=cnorm, hinf=hnorm_inf(csr, dim))


def reference_probes(e):
    """Leg B's unit-vector runs (NPROBE_STEPS steps from e_j, j in
    probe_columns): extended precision and the oracle's f64, H_jj, the
    off-diagonal column norms and the infinity norm of H."""
    return _reference_probes((e.factory, e.sector), e.mode, e.dimup)
