"""Self-energy, Weiss field and bath hybridisation on the device: the second
half of buildGF_impurity (ED_GREENS_FUNCTIONS.f90:22-63), build_sigma_normal
(ED_GF_NORMAL.f90:656-731), build_sigma_superc (ED_GF_SUPERC.f90:826-929) and
build_sigma_nonsu2 (from ED_GF_NONSU2.f90:977), through `ed_sigma_build`
(csrc/ed_sigma.hip).

Sigma is computed block by block; `sigma_blocks` returns the blocks of a
config (`ed_sigma_blocks`: host only, no GPU needed):

    ed_mode  bath_type        blocks
    normal   normal           Nspin*Norb of n = 1
    normal   hybrid, replica  Nspin of n = Norb
    nonsu2   normal           Norb of n = 2 (the two spins of one orbital)
    nonsu2   hybrid, replica  one of n = 2*Norb
    superc   normal           Norb Nambu blocks of n = 2
    superc   hybrid           refused (its orbital off-diagonal G, F are not built)

Every entry outside the blocks is zero in every output.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

import numpy as np

from . import _lib
from ._lib import check
from .gf import GFOptions
from .params import EDConfig

SIGMA_MAX_N, SIGMA_MAX_POLES = 6, 64     # ED_SIGMA_MAX_N, ED_SIGMA_MAX_POLES (include/ed_gpu.h)


class SigmaBlock(ctypes.Structure):
    """ctypes mirror of ``ed_sigma_block`` (include/ed_gpu.h)."""

    _fields_ = [("n", ctypes.c_int32), ("np", ctypes.c_int32), ("nambu", ctypes.c_int32), ("pad_", ctypes.c_int32),
                ("idx", ctypes.c_int32 * SIGMA_MAX_N), ("pad2_", ctypes.c_int32 * 2),
                ("h", ctypes.c_double * (SIGMA_MAX_N * SIGMA_MAX_N * 2)),
                ("e", ctypes.c_double * SIGMA_MAX_POLES),
                ("c", ctypes.c_double * (SIGMA_MAX_POLES * 2)),
                ("w", ctypes.c_double * (SIGMA_MAX_POLES * SIGMA_MAX_N * 2))]


class Block(NamedTuple):
    """One block with numpy views: idx (n,), h (n, n), e (np,), c (np,), w (np, n)."""

    idx: np.ndarray
    nambu: bool
    h: np.ndarray
    e: np.ndarray
    c: np.ndarray
    w: np.ndarray


class Sigma(NamedTuple):
    """impSmats, impSreal, impG0mats, impG0real and the bath's Delta on both
    axes, each (Nspin, Nspin, Norb, Norb, L); for superc also the anomalous
    impSAmats, impSAreal, impF0mats, impF0real (None otherwise)."""

    Smats: object
    Sreal: object
    G0mats: object
    G0real: object
    Dmats: object
    Dreal: object
    SAmats: object = None
    SAreal: object = None
    F0mats: object = None
    F0real: object = None


class BathFunctions(NamedTuple):
    """Delta and G0 (and, for superc, F0) of the bath alone."""

    Dmats: object
    Dreal: object
    G0mats: object
    G0real: object
    F0mats: object = None
    F0real: object = None


def pack_blocks(blocks):
    """A ctypes array of ``ed_sigma_block`` from `Block` tuples."""
    arr = (SigmaBlock * len(blocks))()
    for B, b in zip(arr, blocks):
        n, npole = len(b.idx), len(b.e)
        B.n, B.np, B.nambu = n, npole, int(b.nambu)
        if n > SIGMA_MAX_N or npole > SIGMA_MAX_POLES:
            continue                          # the library refuses the sizes by name
        B.idx[:n] = [int(i) for i in b.idx]
        h = np.zeros((SIGMA_MAX_N, SIGMA_MAX_N), dtype=np.complex128)
        h[:n, :n] = b.h
        w = np.zeros((SIGMA_MAX_POLES, SIGMA_MAX_N), dtype=np.complex128)
        w[:npole, :n] = b.w
        e = np.zeros(SIGMA_MAX_POLES)
        e[:npole] = b.e
        c = np.zeros(SIGMA_MAX_POLES, dtype=np.complex128)
        c[:npole] = b.c
        B.h[:] = h.view(np.float64).ravel().tolist()
        B.e[:] = e.tolist()
        B.c[:] = c.view(np.float64).ravel().tolist()
        B.w[:] = w.view(np.float64).ravel().tolist()
    return arr


def sigma_blocks(cfg: EDConfig):
    """The blocks and pole tables of cfg (host only).  superc with a hybrid
    bath raises NotImplementedError by name."""
    if cfg.ed_mode == "superc" and cfg.bath_type != "normal":
        raise NotImplementedError(f"build_sigma: superc with a {cfg.bath_type} bath is not supported: its orbital "
                                  "off-diagonal G and F are not built (build_gf_superc)")
    p = cfg.to_ctypes()
    arr = (SigmaBlock * (cfg.Nspin * cfg.Norb))()
    nblk = ctypes.c_int32(0)
    check(_lib.load().ed_sigma_blocks(ctypes.byref(p), arr, ctypes.byref(nblk)), "ed_sigma_blocks")
    out = []
    for B in arr[:nblk.value]:
        n, npole = B.n, B.np
        h = np.array(B.h[:]).view(np.complex128).reshape(SIGMA_MAX_N, SIGMA_MAX_N)[:n, :n]
        w = np.array(B.w[:]).view(np.complex128).reshape(SIGMA_MAX_POLES, SIGMA_MAX_N)[:npole, :n]
        out.append(Block(np.array(B.idx[:n]), bool(B.nambu), h.copy(), np.array(B.e[:npole]),
                         np.array(B.c[:]).view(np.complex128)[:npole].copy(), w.copy()))
    return out


def _to_device(a, shape, dev, what):
    import torch

    if a is None:
        return None
    if isinstance(a, torch.Tensor):
        t = a.to(device=dev, dtype=torch.complex128).contiguous()
    else:
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.complex128)).to(dev)
    if tuple(t.shape[:-1]) != shape:
        raise ValueError(f"{what}: shape {tuple(t.shape)} is not (Nspin, Nspin, Norb, Norb, L) = {shape + ('L',)}")
    return t


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else None)


def run_blocks(blocks, nspin, norb, beta, lmats, wini, wfin, lreal, eps, device, Gm=None, Gr=None, Fm=None,
               Fr=None, cfg: Optional[EDConfig] = None):
    """One `ed_sigma_build` (cfg) or `ed_sigma_build_blocks` (an explicit block
    array of `pack_blocks`) call on the current stream.  Returns the ten device
    tensors S, G0, D, SA, F0 on (mats, real), None where not computed."""
    import torch

    if not torch.cuda.is_available():
        raise RuntimeError("the self-energy runs on the GPU (no host fallback)")
    dev = torch.device("cuda", device)
    shape = (nspin, nspin, norb, norb)
    with_g = Gm is not None or Gr is not None
    nambu = Fm is not None or Fr is not None or (cfg is not None and cfg.ed_mode == "superc") or (
        blocks is not None and any(b.nambu for b in blocks))
    g = [_to_device(Gm, shape, dev, "Gmats"), _to_device(Gr, shape, dev, "Greal")]
    f = [_to_device(Fm, shape, dev, "Fmats"), _to_device(Fr, shape, dev, "Freal")]

    def new(L, on):
        return torch.empty(shape + (L,), dtype=torch.complex128, device=dev) if on and L else None

    out = {k: [new(lmats, on), new(lreal, on)]
           for k, on in (("s", with_g), ("g0", True), ("d", True), ("sa", with_g and nambu), ("f0", nambu))}
    st = torch.cuda.current_stream(dev)
    tail = [_ptr(g[0]), _ptr(g[1]), _ptr(f[0]), _ptr(f[1])]
    for k in ("s", "g0", "d", "sa", "f0"):
        tail += [_ptr(out[k][0]), _ptr(out[k][1])]
    tail.append(ctypes.c_void_p(st.cuda_stream))
    lib = _lib.load()
    with torch.cuda.device(dev):
        if cfg is not None:
            p = cfg.to_ctypes()
            check(lib.ed_sigma_build(ctypes.byref(p), float(beta), lmats, float(wini), float(wfin), lreal,
                                     float(eps), *tail), "ed_sigma_build")
        else:
            check(lib.ed_sigma_build_blocks(len(blocks), blocks, nspin, norb, float(beta), lmats, float(wini),
                                            float(wfin), lreal, float(eps), *tail), "ed_sigma_build_blocks")
    # the inputs were read on this stream; the tensors g, f may be freed now
    # (the caching allocator orders the reuse behind the launch)
    return out


def _finish(t, device_out: bool):
    if t is None or device_out:
        return t
    return t.cpu().numpy()


def build_sigma(cfg: EDConfig, Gm, Gr, gopt: Optional[GFOptions] = None, device: int = 0, Fm=None, Fr=None,
                device_out: bool = False) -> Sigma:
    """Sigma = G0^-1 - G^-1, G0 and Delta from the impurity G of `build_gf`
    (and, for superc, the G and F of `build_gf_superc`: without Fm and Fr a
    ValueError).  Gm, Gr (Fm, Fr): numpy arrays or torch device tensors
    (Nspin, Nspin, Norb, Norb, L) on the grids of gopt (`gf.matsubara(gopt.beta,
    L)`, `gf.realaxis(gopt.wini, gopt.wfin, L)`, eps), L taken from the arrays.
    Returns a `Sigma` of numpy arrays, or of torch tensors left in HBM with
    device_out=True.

    superc: the Nambu block of orbital a is [[G, F], [F, -conj(G)]], the last
    entry taken at the mirrored index on the real axis (ED_GF_SUPERC.f90:865-867),
    so the real grid must be symmetric (wini = -wfin) or the call is refused;
    a hybrid bath raises NotImplementedError.

    Where G is a sound input.  Sigma inverts the G it is given, so it is only
    as good as that G.  Two outputs of `build_gf` are not the true Green's
    function and give a Sigma wrong at order 1:
      * a complex impHloc (hybrid / replica baths, or a complex nonsu2 spin
        flip): build_gf copies G_ab into G_ba, which its own docstring says
        holds for a real impHloc_ab only;
      * nonsu2 with a hybrid bath and Norb > 1: the orbital off-diagonal G is
        not built and stays zero.
    These are properties of the input; nothing is refused."""
    gopt = gopt or GFOptions()
    if cfg.ed_mode == "superc":
        if cfg.bath_type != "normal":
            raise NotImplementedError(f"build_sigma: superc with a {cfg.bath_type} bath is not supported: its "
                                      "orbital off-diagonal G and F are not built (build_gf_superc)")
        if Fm is None or Fr is None:
            raise ValueError("build_sigma: ed_mode superc needs the anomalous Fm and Fr of build_gf_superc")
    elif Fm is not None or Fr is not None:
        raise ValueError("build_sigma: Fm / Fr are for ed_mode superc only")
    if Gm is None or Gr is None:
        raise ValueError("build_sigma needs Gm and Gr (bath_functions computes Delta and G0 alone)")
    o = run_blocks(None, cfg.Nspin, cfg.Norb, gopt.beta, int(Gm.shape[-1]), gopt.wini, gopt.wfin, int(Gr.shape[-1]),
                   gopt.eps, device, Gm, Gr, Fm, Fr, cfg=cfg)
    f = [_finish(t, device_out) for k in ("s", "g0", "d", "sa", "f0") for t in o[k]]
    return Sigma(*f)


def bath_functions(cfg: EDConfig, gopt: Optional[GFOptions] = None, device: int = 0,
                   device_out: bool = False) -> BathFunctions:
    """Delta(z) and G0(z) = (z + mu - impHloc - Delta)^-1 of cfg's bath on the
    grids of gopt (Lmats, Lreal points): no G needed.  For superc also F0."""
    gopt = gopt or GFOptions()
    if cfg.ed_mode == "superc" and cfg.bath_type != "normal":
        raise NotImplementedError(f"bath_functions: superc with a {cfg.bath_type} bath is not supported")
    o = run_blocks(None, cfg.Nspin, cfg.Norb, gopt.beta, gopt.Lmats, gopt.wini, gopt.wfin, gopt.Lreal, gopt.eps,
                   device, cfg=cfg)
    f = [_finish(t, device_out) for k in ("d", "g0", "f0") for t in o[k]]
    return BathFunctions(*f)
