"""Self-energy, Weiss field and bath hybridisation on the MI355X: k_sigma<N> /
ed_sigma_build (csrc/ed_sigma.hpp, csrc/ed_sigma.hip) and edgpu.sigma against
numpy and the dense truths of sigma_truth.py.  The bars are those of
tests/test_sigma_cpu.py (its docstring derives them):

  ed_sigma_build against numpy, per block and point, identical inputs:
    |Sigma - Sigma_numpy|_max <= 1e-12 (|invG0|_max + kappa_2(G) |G^-1|_max)
  G0, F0 against the dense truth: <= 1e-13 kappa_2(z - h) max|(z - h)^-1|
  U = 0 identity and the interacting models, per point:
    <= 1e-10 max(|G|, |F|) |G0(z)^-1|_2^2 on the Matsubara axis (1e-5 on the
    real axis of the interacting models: G's own bars through the inverse)
  causality: Im Sigma_aa(i w_n) <= 1e-9.

Measured on the MI355X (largest ratio to each bar): against numpy Sigma 3.8e-4,
G0 7.0e-4, Delta 3.9e-3; U = 0 identity 4.7e-4 (hybrid), G0 / F0 against the
dense truth 3.7e-3; interacting H2 / S1 / N1 (iw) 6.9e-5 / 2.9e-3 / 1.9e-3, (w)
1.3e-8 / 1.1e-8 / 9.0e-6.
"""
import numpy as np
import pytest

import sigma_truth as stt
from edgpu.gf import GFOptions, matsubara, realaxis
from edgpu.params import make_config
from edgpu.sigma import Block, bath_functions, build_sigma, pack_blocks, run_blocks

pytestmark = pytest.mark.gpu

L = 32


def _host(o):
    return {k: tuple(None if t is None else t.cpu().numpy() for t in o[k]) for k in o}


def _run_case(case):
    return run_blocks(pack_blocks(case["blocks"]), case["nspin"], case["norb"], stt.BETA, stt.LM, stt.WINI, stt.WFIN,
                      stt.LR, stt.EPS, 0, Gm=case["G"][0], Gr=case["G"][1], Fm=case["F"][0] if case["F"] else None,
                      Fr=case["F"][1] if case["F"] else None)


@pytest.mark.parametrize("N,npole,nambu", stt.CASES)
def test_ed_sigma_build_against_numpy(N, npole, nambu):
    case = stt.random_case(N, npole, nambu)
    ref, bars = stt.numpy_case(case)
    got, again = _host(_run_case(case)), _host(_run_case(case))
    for k in ("s", "g0", "d") + (("sa", "f0") if nambu else ()):
        for ax in range(2):
            assert np.array_equal(got[k][ax], again[k][ax]), (k, ax)      # two calls: the same bits
    worst, zeros = stt.case_errors(case, got, ref, bars)
    print(f"N={N} poles={npole} nambu={nambu}: ratio to the bar Sigma {worst['s']:.2e} G0 {worst['g0']:.2e} "
          f"Delta {worst['d']:.2e}")
    assert zeros                                                           # exact zeros outside the blocks
    assert worst["s"] <= 1.0 and worst["g0"] <= 1.0 and worst["d"] <= 1.0


def test_mixed_block_sizes_in_one_call():
    """Blocks of n = 1, 2 and 3 in one list: one launch per size, each block
    the same bits as on its own."""
    rng = np.random.default_rng(5)

    def blk(idx):
        n = len(idx)
        h = rng.normal(size=(n, n))
        return Block(np.array(idx), False, (0.2 * (h + h.T)).astype(complex), rng.uniform(-2, 2, 5),
                     np.ones(5, complex), rng.normal(size=(5, n)) + 1j * rng.normal(size=(5, n)))

    blocks = [blk([5]), blk([0, 3]), blk([1, 2, 4])]
    case = stt.random_case(6, 7)
    G = case["G"]

    def run(bl):
        return _host(run_blocks(pack_blocks(bl), 2, 3, stt.BETA, stt.LM, stt.WINI, stt.WFIN, stt.LR, stt.EPS, 0,
                                Gm=G[0], Gr=G[1]))

    both = run(blocks)
    total = {k: [np.zeros_like(both[k][ax]) for ax in range(2)] for k in ("s", "g0", "d")}
    for b in blocks:
        one = run([b])
        for k in total:
            for ax in range(2):
                total[k][ax] += one[k][ax]
    for k in total:
        for ax in range(2):
            assert np.array_equal(both[k][ax], total[k][ax]) and np.any(both[k][ax])


# ------------------------------------------------------------ U = 0 identity
@pytest.mark.parametrize("name", stt.U0_MODELS + stt.U0_SUPERC)
def test_u0_identity_on_the_device_path(name):
    """farm_diag -> build_gf / build_gf_superc -> build_sigma at U = 0: Sigma
    vanishes, G0 and F0 are the dense one-particle / BdG resolvents."""
    from edgpu.diag import DiagOptions
    from edgpu.farm import farm_diag
    from edgpu.gf import build_gf, build_gf_superc
    from edgpu.sectors import get_sector

    cfg = stt.u0_config(name)
    g = GFOptions(Lmats=L, Lreal=L, beta=stt.BETA, eps=stt.EPS, wini=stt.WINI, wfin=stt.WFIN)
    sec = get_sector(cfg)[stt.U0_SECTOR[name]]
    sl = farm_diag(cfg, DiagOptions(), device=0, sectors=[sec.isector]).states
    if cfg.ed_mode == "superc":
        Gm, Gr, Fm, Fr = build_gf_superc(cfg, sl, g)
        F = (Fm, Fr)
        S = build_sigma(cfg, Gm, Gr, g, Fm=Fm, Fr=Fr)
    else:
        Gm, Gr = build_gf(cfg, sl, g)
        F = None
        S = build_sigma(cfg, Gm, Gr, g)
        assert S.SAmats is None and S.F0real is None
    zs = (1j * matsubara(g.beta, L), realaxis(g.wini, g.wfin, L) + 1j * g.eps)
    out = {"s": (S.Smats, S.Sreal), "sa": (S.SAmats, S.SAreal)}
    worst = stt.u0_ratio(cfg, (Gm, Gr), F, out, zs)
    g0w = 0.0
    for ax, z in enumerate(zs):
        D = stt.Dense(cfg, z)
        err = np.max(np.abs((S.G0mats, S.G0real)[ax] - D.g0), axis=(0, 1, 2, 3))
        if F is not None:
            err = np.maximum(err, np.max(np.abs((S.F0mats, S.F0real)[ax] - D.f0), axis=(0, 1, 2, 3)))
        g0w = max(g0w, float(np.max(err / (1e-13 * D.bar))))
    print(f"{name}: sector {stt.U0_SECTOR[name]} ({sec.dim} rows), {sl.size} state(s): |Sigma| ratio to the bar "
          f"{worst:.2e}; G0 against the dense truth {g0w:.2e}")
    assert worst <= 1.0
    assert g0w <= 1.0


# ------------------------------------------------------- interacting models
@pytest.mark.parametrize("name", stt.INTERACTING)
def test_interacting_sigma_against_the_dense_truth(name):
    from edgpu.diag import DiagOptions
    from edgpu.farm import farm_diag
    from edgpu.gf import build_gf, build_gf_superc

    cfg, eps = stt.interacting_config(name)
    g = GFOptions(Lmats=L, Lreal=L, beta=stt.BETA, eps=eps, wini=stt.WINI, wfin=stt.WFIN)
    wm, wr = matsubara(g.beta, L), realaxis(g.wini, g.wfin, L)
    sl = farm_diag(cfg, DiagOptions(), device=0).states
    if cfg.ed_mode == "superc":
        Gm, Gr, Fm, Fr = build_gf_superc(cfg, sl, g)
        S = build_sigma(cfg, Gm, Gr, g, Fm=Fm, Fr=Fr)
    else:
        Gm, Gr = build_gf(cfg, sl, g)
        S = build_sigma(cfg, Gm, Gr, g)
    Gt, Ft = stt.interacting_truth(name, sl, wm, wr, eps)
    rm, rr, im, smax = stt.interacting_ratios(cfg, Gt, Ft, (S.Smats, S.Sreal), (S.SAmats, S.SAreal),
                                              (1j * wm, wr + 1j * eps))
    print(f"{name}: {sl.size} state(s), eps {eps}: ratio to the bar (iw) {rm:.2e} (w) {rr:.2e}; "
          f"max Im Sigma_aa(iw) {im:.2e}; max|Sigma| {smax:.2f}")
    assert smax > 0.1
    assert rm <= 1.0 and rr <= 1.0
    assert im <= 1e-9                                                      # causality


# ---------------------------------------------------------------- API checks
def test_device_out_and_bath_functions():
    import torch

    cfg = stt.u0_config("hybrid")
    g = GFOptions(Lmats=L, Lreal=L, beta=stt.BETA, eps=stt.EPS)
    case = stt.random_case(6, 7)
    Gm = np.ascontiguousarray(case["G"][0][:1, :1, :2, :2, :L])
    Gr = np.ascontiguousarray(case["G"][1][:1, :1, :2, :2, :L])
    host = build_sigma(cfg, Gm, Gr, g)
    dev = build_sigma(cfg, torch.from_numpy(Gm).cuda(), torch.from_numpy(Gr).cuda(), g, device_out=True)
    for a, b in zip(host[:6], dev[:6]):
        assert isinstance(a, np.ndarray) and isinstance(b, torch.Tensor) and b.is_cuda
        assert a.shape == (1, 1, 2, 2, L) and np.array_equal(a, b.cpu().numpy()) and np.any(a)
    assert all(t is None for t in host[6:]) and all(t is None for t in dev[6:])
    bf = bath_functions(cfg, g)
    assert np.array_equal(bf.Dmats, host.Dmats) and np.array_equal(bf.G0real, host.G0real) and bf.F0mats is None
    sc = stt.u0_config("superc_1")
    bs = bath_functions(sc, g)
    assert bs.F0mats.shape == (1, 1, 1, 1, L) and np.any(bs.F0real)


def test_refusals():
    sc = stt.u0_config("superc_1")
    z = np.zeros((1, 1, 1, 1, 8), dtype=np.complex128)
    with pytest.raises(ValueError, match="Fm"):
        build_sigma(sc, z + 1.0, z + 1.0, GFOptions())
    with pytest.raises(Exception, match="symmetric"):
        build_sigma(sc, z + 1.0, z + 1.0, GFOptions(wini=-5.0, wfin=4.0), Fm=z + 0.1, Fr=z + 0.1)
    sh_cfg = make_config(Norb=2, Nbath=2, Nspin=1, ed_mode="superc", bath_type="hybrid", bath="random", seed=31)
    z2 = np.zeros((1, 1, 2, 2, 8), dtype=np.complex128)
    with pytest.raises(NotImplementedError, match="superc with a hybrid bath"):
        build_sigma(sh_cfg, z2, z2, GFOptions(), Fm=z2, Fr=z2)
    with pytest.raises(NotImplementedError, match="superc with a hybrid bath"):
        bath_functions(sh_cfg, GFOptions(Lmats=4, Lreal=4))
    with pytest.raises(ValueError, match="shape"):
        build_sigma(stt.u0_config("hybrid"), z, z, GFOptions())
