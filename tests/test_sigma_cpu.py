"""Self-energy and Weiss field on the CPU: the host half of the kernel
(csrc/ed_sigma_host.hpp: sigma_blocks, sigma_compile, sigma_point, sigma_host)
through the stand-alone g++ driver of sigma_host.py, against numpy and against
the dense one-particle and Bogoliubov-de Gennes truths of sigma_truth.py.

Bars (derived, not measured).
  sigma_host against numpy, per block and grid point, identical inputs:
    |Sigma - Sigma_numpy|_max <= 1e-12 (|invG0|_max + kappa_2(G) |G^-1|_max),
  the forward-error bound of pivoted elimination at n <= 6 with about 100x
  headroom (G0: 1e-12 kappa_2(invG0) |G0|_max; Delta: 1e-13 sum_p |term_p|).
  G0 (and F0) against the dense truth, per point:
    <= 1e-13 kappa_2(z - h) max|(z - h)^-1|.
  U = 0 identity through the oracle pipeline, per point:
    |Sigma|, |Sigma_A| <= 1e-10 max(|G|, |F|) |G0(z)^-1|_2^2,
  the project's 1e-10 bar on G carried through the inverse; the oracle path
  must sit 10x inside it.

Largest ratios to the bars seen here: sigma_host against numpy Sigma 3.8e-4,
G0 7.0e-4, Delta 3.9e-3 (15 cases plus 3 Nambu ones); G0 against the dense
truth 4.7e-3 (seven models, both axes); U = 0 identity 1.2e-3; interacting
H2 / S1 / N1 (iw) 3.7e-4 / 5.3e-3 / 3.6e-4, (w) 1.4e-8 / 3.9e-8 / 1.1e-5.
"""
import numpy as np
import pytest

import cases
import sigma_host as sh
import sigma_truth as stt
from edgpu.gf import GFOptions, matsubara, realaxis
from edgpu.params import make_config
from edgpu.sigma import Block, pack_blocks

ED_ERR_ARG, ED_ERR_UNSUPPORTED = 1, 5


@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    d = tmp_path_factory.mktemp("sigma")
    return sh.build(d), d


def _summary(arr):
    return [(B.n, B.np, B.nambu, list(B.idx[:B.n])) for B in arr]


# ------------------------------------------------------------------ block list
def _pairs():
    n3 = cases.normal_3orb()                                             # normal / normal, Nspin = 2, Norb = 3
    hy = cases.hybrid()                                                  # normal / hybrid, Nspin = 1, Norb = 2
    h3 = make_config(Norb=3, Nbath=2, Nspin=2, bath_type="hybrid", bath="random", seed=21)
    rc = cases.replica_cplx()                                            # normal / replica, complex blocks
    nn = cases.nonsu2_rand()                                             # nonsu2 / normal, Norb = 2
    nh = make_config(Norb=2, Nbath=3, Nspin=2, ed_mode="nonsu2", bath_type="hybrid", bath="random", seed=5)
    nr = cases.nonsu2_jz()                                               # nonsu2 / replica, Norb = 3
    sc = cases.superc_2orb()                                             # superc / normal
    return [
        ("normal/normal", n3, [(1, 1, 0, [i]) for i in range(6)]),
        ("normal/hybrid", hy, [(2, 4, 0, [0, 1])]),
        ("normal/hybrid Nspin=2", h3, [(3, 2, 0, [0, 1, 2]), (3, 2, 0, [3, 4, 5])]),
        ("normal/replica", rc, [(2, 2 * 2 * 2, 0, [0, 1])]),             # complex blocks: 2n poles each
        ("nonsu2/normal", nn, [(2, 4, 0, [0, 2]), (2, 4, 0, [1, 3])]),
        ("nonsu2/hybrid", nh, [(4, 6, 0, [0, 1, 2, 3])]),
        ("nonsu2/replica", nr, [(6, 6, 0, [0, 1, 2, 3, 4, 5])]),         # real blocks: n poles each
        ("superc/normal", sc, [(2, 4, 1, [0, 0]), (2, 4, 1, [1, 1])]),
    ]


def test_block_list_of_every_mode_and_bath(drv):
    exe, d = drv
    for name, cfg, want in _pairs():
        rc, msg, arr, n = sh.blocks_of(exe, cfg, d)
        assert rc == 0 and _summary(arr) == want, (name, rc, msg, arr and _summary(arr))
    sh_cfg = make_config(Norb=2, Nbath=2, Nspin=1, ed_mode="superc", bath_type="hybrid", bath="random", seed=31)
    rc, msg, arr, n = sh.blocks_of(exe, sh_cfg, d)
    assert rc == ED_ERR_UNSUPPORTED and "superc" in msg and "hybrid" in msg and arr is None


def test_library_export_gives_the_same_blocks(drv):
    """ed_sigma_blocks of the shared library (host only, no GPU needed)."""
    from edgpu.sigma import sigma_blocks

    exe, d = drv
    for name, cfg, want in _pairs():
        got = sigma_blocks(cfg)
        assert [(len(b.idx), len(b.e), int(b.nambu), list(b.idx)) for b in got] == want, name
        _, _, arr, _ = sh.blocks_of(exe, cfg, d)
        for b, B in zip(got, arr):
            assert np.array_equal(b.e, np.array(B.e[:B.np]))
    with pytest.raises(Exception, match="superc"):
        sigma_blocks(make_config(Norb=2, Nbath=2, Nspin=1, ed_mode="superc", bath_type="hybrid", bath="random"))


def test_superc_poles_are_the_bogoliubov_pairs(drv):
    exe, d = drv
    cfg = cases.superc()
    _, _, arr, n = sh.blocks_of(exe, cfg, d)
    B = arr[0]
    e = np.array(B.e[:B.np])
    want = np.sqrt(cfg.bath.e[0, 0] ** 2 + cfg.bath.d[0, 0] ** 2)
    assert np.allclose(e[0::2], want, rtol=1e-15) and np.array_equal(e[1::2], -e[0::2])
    w = np.array(B.w[:]).reshape(64, 6, 2)[:B.np, :2, 0]
    # the two poles of one bath level carry V^2 on the particle and on the hole
    assert np.allclose(w[0::2] ** 2 + w[1::2] ** 2, (cfg.bath.v[0, 0] ** 2)[:, None], rtol=1e-14)


# --------------------------------------------------------------------- refusals
def _one(n=1, npole=1, idx=None, nambu=False):
    idx = list(range(n)) if idx is None else idx
    return Block(np.array(idx), nambu, np.zeros((len(idx), len(idx)), complex), np.linspace(-1, 1, npole),
                 np.ones(npole, complex), np.full((npole, len(idx)), 0.3, complex))


def test_refusals_of_sigma_compile(drv):
    exe, d = drv

    def code(blocks, nspin=2, norb=3, wini=-5.0, wfin=5.0, lreal=5, G=None):
        rc, msg, out = sh.run(exe, d, pack_blocks(blocks), nspin, norb, 10.0, 4, wini, wfin, lreal, 0.1, G=G,
                              tag="ref")
        return rc, msg

    assert code([_one(1, 3)])[0] == 0
    for n in (0, 5, 7):
        b = _one(1, 3)
        arr = pack_blocks([b])
        arr[0].n = n
        rc, msg, _ = sh.run(exe, d, arr, 2, 3, 10.0, 4, -5.0, 5.0, 5, 0.1, tag="ref")
        assert rc == ED_ERR_ARG and "block size" in msg, (n, rc, msg)
    for npole in (0, 65):
        arr = pack_blocks([_one(1, 3)])
        arr[0].np = npole
        rc, msg, _ = sh.run(exe, d, arr, 2, 3, 10.0, 4, -5.0, 5.0, 5, 0.1, tag="ref")
        assert rc == ED_ERR_ARG and "pole count" in msg, (npole, rc, msg)
    assert code([_one(1, 64)])[0] == 0
    rc, msg = code([_one(2, 2, [0, 1]), _one(2, 2, [1, 2])])
    assert rc == ED_ERR_ARG and "overlapping" in msg
    rc, msg = code([_one(2, 2, [0, 0])])
    assert rc == ED_ERR_ARG and "overlapping" in msg
    assert code([_one(1, 2, [6])])[0] == ED_ERR_ARG                     # index outside the impurity
    # superc: a symmetric real grid or none
    nb = [_one(2, 2, [1, 1], nambu=True)]
    assert code(nb, nspin=1)[0] == 0
    rc, msg = code(nb, nspin=1, wini=-5.0, wfin=4.0)
    assert rc == ED_ERR_ARG and "symmetric" in msg
    assert code(nb, nspin=1, wini=-5.0, wfin=4.0, lreal=0)[0] == 0      # no real axis: nothing to mirror
    assert code(nb, nspin=2)[0] == ED_ERR_ARG                           # a Nambu block needs Nspin = 1
    # aliasing
    rows = sh.alias_codes(exe)
    assert [int(r[0]) for r in rows] == [0, 1, 1, 1, 1, 0], rows
    assert all("alias" in r[1] for r in rows[1:5])


# ------------------------------------------------------- sigma_host against numpy
CASES = stt.CASES


def _host_case(exe, d, case, tag="case"):
    rc, msg, out = sh.run(exe, d, pack_blocks(case["blocks"]), case["nspin"], case["norb"], stt.BETA, stt.LM, stt.WINI,
                          stt.WFIN, stt.LR, stt.EPS, G=case["G"], F=case["F"], tag=tag)
    assert rc == 0, msg
    return out


@pytest.mark.parametrize("N,npole,nambu", CASES)
def test_sigma_host_against_numpy(drv, N, npole, nambu):
    exe, d = drv
    case = stt.random_case(N, npole, nambu)
    ref, bars = stt.numpy_case(case)
    got = _host_case(exe, d, case)
    worst, zeros = stt.case_errors(case, got, ref, bars)
    smax = max(np.max(np.abs(ref["s"][ax])) for ax in range(2))
    print(f"N={N} poles={npole} nambu={nambu}: ratio to the bar Sigma {worst['s']:.2e} G0 {worst['g0']:.2e} "
          f"Delta {worst['d']:.2e}; max|Sigma| {smax:.2e}")
    assert smax > 0.1                                # a genuine self-energy, not a difference of equals
    assert zeros
    assert worst["s"] <= 1.0 and worst["g0"] <= 1.0 and worst["d"] <= 1.0


def test_grid_is_the_python_grid_bit_for_bit(drv):
    """Delta of one pole at e = 0 with weight 1 is 1 / z: z comes back exactly."""
    exe, d = drv
    b = Block(np.array([0]), False, np.zeros((1, 1), complex), np.zeros(1), np.ones(1, complex), np.ones((1, 1), complex))
    for (beta, lm, wini, wfin, lr) in ((50.0, 67, -5.0, 5.0, 65), (7.3, 5, -1.7, 2.9, 4), (1000.0, 3, 0.0, 1.0, 1)):
        rc, msg, out = sh.run(exe, d, pack_blocks([b]), 1, 1, beta, lm, wini, wfin, lr, 0.25, tag="grid")
        assert rc == 0
        zm, zr = 1.0 / out["d"][0][0, 0, 0, 0], 1.0 / out["d"][1][0, 0, 0, 0]
        assert np.allclose(zm.imag, matsubara(beta, lm), rtol=4e-16, atol=0) and np.all(np.abs(zm.real) < 1e-300)
        assert np.allclose(zr.real, realaxis(wini, wfin, lr), rtol=4e-16, atol=1e-16)


# ------------------------------------------------------- G0 against the dense truth
@pytest.mark.parametrize("name", stt.U0_MODELS + stt.U0_SUPERC)
def test_g0_against_the_dense_truth(drv, name):
    exe, d = drv
    cfg = stt.u0_config(name)
    if cfg.ed_mode == "superc":
        assert stt.h_bdg(cfg)[1] < 1e-15             # the Nambu states span an invariant subspace
    rc, msg, arr, n = sh.blocks_of(exe, cfg, d)
    assert rc == 0, msg
    rc, msg, out = sh.run(exe, d, arr, cfg.Nspin, cfg.Norb, stt.BETA, stt.LM, stt.WINI, stt.WFIN, stt.LR, stt.EPS,
                          tag="g0")
    assert rc == 0, msg
    worst = 0.0
    for ax, z in enumerate(stt.case_grids()):
        D = stt.Dense(cfg, z)
        err = np.max(np.abs(out["g0"][ax] - D.g0), axis=(0, 1, 2, 3))
        if cfg.ed_mode == "superc":
            err = np.maximum(err, np.max(np.abs(out["f0"][ax] - D.f0), axis=(0, 1, 2, 3)))
            assert np.max(np.abs(D.f0)) > 0.1
        worst = max(worst, float(np.max(err / (1e-13 * D.bar))))
        assert not np.any(out["s"][ax])              # no G given: Sigma is not computed
    print(f"{name}: G0 against the dense truth, ratio to the bar {worst:.2e}")
    assert worst <= 1.0


def test_complex_replica_vr_follows_the_library_hamiltonian(drv):
    """A complex vr enters H conjugated in both hopping directions (cases.
    replica_cplx_vr), so Delta = conj(vr)^2 (z - h_k)^-1, not |vr|^2: G0 is the
    resolvent of the one-particle block of the oracle's own H."""
    from oracle.oracle import Oracle, spmv

    exe, d = drv
    cfg = stt.noninteracting(cases.replica_cplx_vr())
    orc = Oracle(cfg)

    def dense(q1, q2):
        hmap = orc.build_sector(q1, q2)
        csr = orc.build_csr(hmap)
        return hmap, np.array([spmv(csr, col) for col in np.eye(len(hmap))]).T

    hmap, h = dense(1, 0)                            # one up electron: the one-particle block
    h = h - dense(0, 0)[1][0, 0] * np.eye(len(hmap))
    lev = [int(m).bit_length() - 1 for m in hmap]
    assert np.max(np.abs(h - h.conj().T)) > 0.05     # complex-symmetric, not Hermitian
    rc, msg, arr, n = sh.blocks_of(exe, cfg, d)
    rc, msg, out = sh.run(exe, d, arr, 1, 2, stt.BETA, 16, stt.WINI, stt.WFIN, 15, stt.EPS, tag="vr")
    imp = [lev.index(o) for o in range(cfg.Norb)]
    for ax, z in enumerate((1j * matsubara(stt.BETA, 16), realaxis(stt.WINI, stt.WFIN, 15) + 1j * stt.EPS)):
        R = np.linalg.inv(z[:, None, None] * np.eye(len(hmap))[None] - h[None])
        want = np.moveaxis(R[:, imp][:, :, imp], 0, -1)
        # kappa(z - h) <= |z - h| / eps ~ 200 here: 1e-12 is some 10x above 200 * 2^-53 * a few
        assert np.max(np.abs(out["g0"][ax][0, 0] - want)) < 1e-12 * np.max(np.abs(want))


# ----------------------------------------------- U = 0 identity, oracle pipeline
@pytest.mark.parametrize("name", stt.U0_MODELS + stt.U0_SUPERC)
def test_u0_identity_through_the_oracle_pipeline(drv, name):
    from edgpu.diag import DiagOptions
    from edgpu.farm import farm_diag
    from edgpu.gf import build_gf, build_gf_superc
    from edgpu.sectors import get_sector
    from oracle_gf import oracle_job_runner
    from oracle_gf_superc import oracle_job_runner_superc
    from oracle_solver import solve_sector_oracle

    exe, d = drv
    cfg = stt.u0_config(name)
    L = 32
    g = GFOptions(Lmats=L, Lreal=L, beta=stt.BETA, eps=stt.EPS, wini=stt.WINI, wfin=stt.WFIN)
    sec = get_sector(cfg)[stt.U0_SECTOR[name]]
    sl = farm_diag(cfg, DiagOptions(lanc_method="lanczos"), solver=solve_sector_oracle, sectors=[sec.isector]).states
    if cfg.ed_mode == "superc":
        Gm, Gr, Fm, Fr = build_gf_superc(cfg, sl, g, runner=oracle_job_runner_superc)
        F = (Fm, Fr)
    else:
        Gm, Gr = build_gf(cfg, sl, g, runner=oracle_job_runner)
        F = None
    _, _, arr, _ = sh.blocks_of(exe, cfg, d)
    rc, msg, out = sh.run(exe, d, arr, cfg.Nspin, cfg.Norb, g.beta, L, g.wini, g.wfin, L, g.eps, G=(Gm, Gr), F=F,
                          tag="u0")
    assert rc == 0, msg
    worst = stt.u0_ratio(cfg, (Gm, Gr), F, out, (1j * matsubara(g.beta, L), realaxis(g.wini, g.wfin, L) + 1j * g.eps))
    print(f"{name}: U = 0, |Sigma| against 1e-10 max(|G|, |F|) |G0^-1|_2^2: ratio {worst:.2e}")
    assert worst <= 0.1                              # the oracle path sits 10x inside the bar


# ------------------------------------------------------------------- sanitizers
def test_driver_clean_under_sanitizers(drv):
    """The same driver under AddressSanitizer + UBSan (host code with its own
    main, run as a child process): no report, the same bytes."""
    exe, d = drv
    san = sh.build(d, ("-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    for N, npole, nambu in ((6, 64, False), (4, 7, False), (3, 1, False), (1, 64, False), (2, 7, True)):
        case = stt.random_case(N, npole, nambu)
        a, b = _host_case(exe, d, case, "plain"), _host_case(san, d, case, "san")
        for k in sh.OUT_KEYS:
            for ax in range(2):
                assert np.array_equal(a[k][ax], b[k][ax]), (N, npole, k, ax)
    for cfg in (cases.replica_cplx(), cases.nonsu2_jz(), cases.superc_2orb(), cases.nonsu2_rand()):
        x, y = sh.blocks_of(exe, cfg, d, "plain"), sh.blocks_of(san, cfg, d, "san")
        assert x[0] == y[0] == 0 and bytes(x[2]) == bytes(y[2])
    assert sh.alias_codes(san) == sh.alias_codes(exe)


# ------------------------------------------ interacting models, oracle pipeline
@pytest.mark.parametrize("name", stt.INTERACTING)
def test_interacting_sigma_through_the_oracle_pipeline(drv, name):
    """Sigma of H2, S1 and N1 against G0_truth^-1 - G_Lehmann^-1 at the bars
    of the device test (tests/test_gpu_sigma.py), with the oracle's G."""
    from edgpu.diag import DiagOptions
    from edgpu.farm import farm_diag
    from edgpu.gf import build_gf, build_gf_superc
    from oracle_gf import oracle_job_runner
    from oracle_gf_superc import oracle_job_runner_superc
    from oracle_solver import solve_sector_oracle

    exe, d = drv
    cfg, eps = stt.interacting_config(name)
    L = 32
    g = GFOptions(Lmats=L, Lreal=L, beta=stt.BETA, eps=eps, wini=stt.WINI, wfin=stt.WFIN)
    wm, wr = matsubara(g.beta, L), realaxis(g.wini, g.wfin, L)
    sl = farm_diag(cfg, DiagOptions(lanc_method="lanczos"), solver=solve_sector_oracle).states
    if cfg.ed_mode == "superc":
        Gm, Gr, Fm, Fr = build_gf_superc(cfg, sl, g, runner=oracle_job_runner_superc)
        F = (Fm, Fr)
    else:
        Gm, Gr = build_gf(cfg, sl, g, runner=oracle_job_runner)
        F = None
    _, _, arr, _ = sh.blocks_of(exe, cfg, d)
    rc, msg, out = sh.run(exe, d, arr, cfg.Nspin, cfg.Norb, g.beta, L, g.wini, g.wfin, L, g.eps, G=(Gm, Gr), F=F,
                          tag="int")
    assert rc == 0, msg
    Gt, Ft = stt.interacting_truth(name, sl, wm, wr, eps)
    rm, rr, im, smax = stt.interacting_ratios(cfg, Gt, Ft, out["s"], out["sa"], (1j * wm, wr + 1j * eps))
    print(f"{name}: {sl.size} state(s), eps {eps}: ratio to the bar (iw) {rm:.2e} (w) {rr:.2e}; "
          f"max Im Sigma_aa(iw) {im:.2e}; max|Sigma| {smax:.2f}")
    assert smax > 0.1
    assert rm <= 1.0 and rr <= 1.0
    assert im <= 1e-9
