"""Every launch form of the persistent Lanczos kernel outside real-vector
MODE 4 (the table and its coverage list: tests/persist_shape_cases.py; the
references' own margins: tests/test_persist_shapes_cpu.py).

A. Sector.lanc_geom (the library's answer, not the table's mirror) names the
   entry's form; alpha / beta of the first m = min(24, dim // 2) steps agree
   with the extended-precision recurrence on the oracle's CSR at the
   project's Lanczos bars (rtol 1e-10, atol 1e-12), nlanc with the oracle's,
   and min(40, dim // 2) steps with the multi-kernel recurrence at rtol 1e-9,
   atol 1e-11.
B. Unit start vectors e_j in batched launches (at most 96 seeds each), three
   steps (alpha[0..1] and beta[1..2] are the first two; beta[2] needs the
   third slot): a row slot, padding word or dictionary entry that is wrong
   for one row shows at that row.  With s = 1 and b = 0 nothing rounds in
   alpha[0] = H_jj: bit for bit the oracle's in the stored forms.  The
   matrix-free forms (modes 1 and 3, MODE 4 without a stored matrix) generate
   the diagonal as aup + adw + U from the Kronecker tables, a sum of the same
   terms in another order than the oracle's, which the project holds to 1e-13
   (tests/test_gpu_hxv.py): there alpha[0] equals bit for bit the diagonal of
   the library's own matrix-free Kronecker H.v (k_kron, the same expression),
   and the oracle's H_jj within 1e-13 * |H|_inf.  beta[1] is the column's
   off-diagonal 2-norm, a sum of at most 20 squares and a root (error below
   3e-15; bar 1e-14 relative); alpha[1] and beta[2] within 1e-12 * |H|_inf of
   the extended-precision values (a missing conjugate of a complex H shows
   in alpha[1]).
C. The launch path (tests/test_gpu_persist_launch.py's legs) on one padded
   entry per (mode, HC, VC), bit for bit where the same kernel runs on the
   same numbers; the continuation launch (first = 0: R and P reloaded, P from
   global memory in the register modes with complex vectors) through
   lanc_eigh.
"""
import numpy as np
import pytest

import persist_mode4_cases as pc
import persist_shape_cases as ps

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _open(e):
    from edgpu.hamiltonian import Sector

    return Sector(e.factory(), e.sector[0], e.sector[1], options=e.options, **e.kw)


def _dev(v):
    t = torch.from_numpy(np.ascontiguousarray(v)).to("cuda:0").contiguous()
    torch.cuda.synchronize()
    return t


def _same(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    bad = np.nonzero(pc.bits(got).ravel() != pc.bits(want).ravel())[0]
    assert bad.size == 0, (what, "first differing entry", int(bad[0]), got.ravel()[bad[0]], want.ravel()[bad[0]])


def _zeros(x, what):
    _same(x, np.zeros(np.shape(x)), what)     # exactly +0.0


def _batch(S, seeds, n, e, threshold=1e-13):
    from edgpu.gf import _tridiag_batch

    dt = np.complex128 if e.vc else np.float64
    return _tridiag_batch(S, _dev(np.ascontiguousarray(seeds, dtype=dt)), n, not e.vc, threshold)


def _assert_geom(S, e):
    g = S.lanc_geom(real=not e.vc)
    assert (g["mode"], g["hc"], e.vc, g["width"], g["rpt"]) == ps.form(e), g
    assert g["threads"] == ps.nthreads(e.mode) and g["lds"] > 0
    assert S.lanc_mode(real=not e.vc) == e.mode
    assert S.dim == e.dim
    if not e.kw["stored"]:
        assert S.info.kron == 1
        assert int(S.info.dimup) == e.dimup


def _kron_diagonal(S, e, cols):
    """H_jj as the matrix-free Kronecker H.v (path 2) generates it: row j of
    H e_j, where the off-diagonal terms multiply zeros."""
    x = torch.zeros(e.dim, dtype=torch.complex128 if e.vc else torch.float64, device="cuda:0")
    out = torch.empty_like(x)
    d = np.zeros(len(cols))
    for n, j in enumerate(cols.tolist()):
        x[j] = 1.0
        torch.cuda.synchronize()
        S.hxv_dev(x, out, path=2)
        torch.cuda.synchronize()
        v = out[j].item()
        assert np.imag(v) == 0.0
        d[n] = np.real(v)
        x[j] = 0.0
    return d


@pytest.fixture(scope="module", params=ps.TABLE, ids=ps.IDS)
def shape(request):
    e = request.param
    with _open(e) as S:
        yield e, S


def test_recurrence_against_reference(shape):
    e, S = shape
    real = not e.vc
    _assert_geom(S, e)
    r = ps.reference_run(e)
    n, m, v0 = r["n"], r["m"], r["v0"]
    a, b, ng = S.lanc_tridiag(v0, n, real=real)
    ax = np.asarray(r["ext"][0], dtype=np.float64)
    bx = np.asarray(r["ext"][1], dtype=np.float64)
    print(e.id, "vs reference: max |d alpha| %.3e  max |d beta| %.3e over %d steps" %
          (np.max(np.abs(a[:m] - ax[:m])), np.max(np.abs(b[:m] - bx[:m])), m))
    assert ng == r["oracle"][2]
    assert b[0] == 0.0
    np.testing.assert_allclose(a[:m], ax[:m], rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(b[:m], bx[:m], rtol=1e-10, atol=1e-12)
    S.set_options(*e.options, "no_persist")
    try:
        assert S.lanc_geom(real=real)["mode"] == -1
        a2, b2, n2 = S.lanc_tridiag(v0, n, real=real)
    finally:
        S.set_options(*e.options)
    print(e.id, "vs multi-kernel: max |d alpha| %.3e  max |d beta| %.3e over %d steps" %
          (np.max(np.abs(a - a2)), np.max(np.abs(b - b2)), n))
    assert n2 == ng
    np.testing.assert_allclose(a[:n], a2[:n], rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(b[:n], b2[:n], rtol=1e-9, atol=1e-11)


def test_column_probes(shape):
    e, S = shape
    _assert_geom(S, e)
    p = ps.reference_probes(e)
    cols = p["cols"]
    k = len(cols)
    a = np.zeros((k, ps.NPROBE_STEPS))
    b = np.zeros((k, ps.NPROBE_STEPS))
    nl = np.zeros(k, dtype=np.int64)
    for c0 in range(0, k, ps.NPROBE_MAX):
        part = cols[c0:c0 + ps.NPROBE_MAX]
        seeds = np.zeros((len(part), e.dim))
        seeds[np.arange(len(part)), part] = 1.0
        a[c0:c0 + len(part)], b[c0:c0 + len(part)], nl[c0:c0 + len(part)] = _batch(S, seeds, ps.NPROBE_STEPS, e)
    ax, bx, nx = p["ext"]
    hinf = p["hinf"]
    d1 = np.abs(a[:, 1] - np.asarray(ax[:, 1], dtype=np.float64))
    d2 = np.abs(b[:, 2] - np.asarray(bx[:, 2], dtype=np.float64))
    cn = np.asarray(p["cnorm"], dtype=np.float64)
    rb = np.abs(b[:, 1] - cn) / np.where(cn > 0, cn, 1.0)
    print(e.id, "%d probes: beta[1] rel %.3e, alpha[1] %.3e, beta[2] %.3e of |H|_inf %.3f" %
          (k, rb.max(), d1.max() / hinf, d2.max() / hinf, hinf))
    assert np.array_equal(nl, nx), cols[np.nonzero(nl != nx)[0]]
    if e.kw["stored"]:
        hjj = p["hjj"]
    else:
        hjj = _kron_diagonal(S, e, cols)
        dd = np.abs(hjj - p["hjj"])
        print(e.id, "generated diagonal against the oracle's: %.3e of |H|_inf" % (dd.max() / hinf))
        assert np.all(dd <= 1e-13 * hinf), ("generated H_jj at columns", cols[dd > 1e-13 * hinf])
    bad = np.nonzero(pc.bits(a[:, 0]) != pc.bits(hjj))[0]
    assert bad.size == 0, ("alpha[0] != H_jj at columns", cols[bad], a[bad, 0], hjj[bad])
    _zeros(b[:, 0], "beta[0]")
    assert np.all(rb <= 1e-14), ("beta[1] at columns", cols[rb > 1e-14], rb[rb > 1e-14])
    assert np.all(d1 <= 1e-12 * hinf), ("alpha[1] at columns", cols[d1 > 1e-12 * hinf], d1[d1 > 1e-12 * hinf])
    assert np.all(d2 <= 1e-12 * hinf), ("beta[2] at columns", cols[d2 > 1e-12 * hinf], d2[d2 > 1e-12 * hinf])


# ------------------------------------------------------------- C. launch path
LAUNCH = ps.launch_entries()
NLONG, NSHORT = 60, 10


def _start2(e, k):
    i = np.arange(1, e.dim + 1, dtype=np.float64)
    return (np.sin(k * i) + 1j * np.cos((k + 2) * i)) if e.vc else np.sin(k * i)


@pytest.fixture(scope="module", params=LAUNCH, ids=[e.id for e in LAUNCH])
def launch(request):
    """One sector per (mode, HC, VC) with the run every leg compares against."""
    e = request.param
    with _open(e) as S:
        _assert_geom(S, e)
        v0 = ps.start(e, e.dim)
        ref = S.lanc_tridiag(v0, NLONG, real=not e.vc)
        assert ref[2] == NLONG
        yield e, S, v0, ref


def test_lanc_run_matches_tridiag_and_leaves_start_vector(launch):
    e, S, v0, (a, b, _) = launch
    d = _dev(v0)
    before = d.clone()
    ar, br, _ = S.lanc_run(NLONG, v0_dev=d)
    torch.cuda.synchronize()
    _same(ar, a, "alpha")
    _same(br, b, "beta")
    _zeros(br[:1], "beta[0]")
    raw = (lambda t: torch.view_as_real(t) if t.is_complex() else t)
    assert torch.equal(raw(d).view(torch.int64), raw(before).view(torch.int64)), "start vector written"
    _same(raw(d).cpu().numpy(), raw(_dev(v0)).cpu().numpy(), "start vector")


def test_short_run_after_a_long_one(launch):
    e, S, v0, (a, b, _) = launch
    d, other = _dev(v0), _dev(_start2(e, 2))
    ao, bo, _ = S.lanc_run(NLONG, v0_dev=other)
    assert not np.array_equal(pc.bits(ao), pc.bits(a))
    short = S.lanc_run(NSHORT, v0_dev=d)
    _same(short[0], a[:NSHORT], "alpha, short run after a long one")
    _same(short[1], b[:NSHORT], "beta, short run after a long one")
    at, bt, nt = S.lanc_tridiag(v0, NSHORT, real=not e.vc)
    assert nt == NSHORT
    _same(at, a[:NSHORT], "alpha, short lanc_tridiag")
    _same(bt, b[:NSHORT], "beta, short lanc_tridiag")
    r3 = S.lanc_run(NLONG, v0_dev=d)
    _same(r3[0], a, "alpha, long run again")
    _same(r3[1], b, "beta, long run again")


def test_zero_start_vector_after_a_longer_run(launch):
    e, S, v0, (a, b, _) = launch
    real = not e.vc
    d = _dev(v0)
    S.lanc_run(NLONG, v0_dev=d)                      # leaves NLONG steps of alpha / beta behind
    z = np.zeros(e.dim, dtype=v0.dtype)
    az, bz, nz = S.lanc_tridiag(z, NLONG, real=real)
    assert nz == 0
    _zeros(az, "alpha of the zero vector")
    _zeros(bz, "beta of the zero vector")
    S.lanc_run(NLONG, v0_dev=d)
    ar, br, _ = S.lanc_run(NLONG, v0_dev=_dev(z))    # unmasked: the kernel's own zeros
    _zeros(ar, "alpha of the zero vector, lanc_run")
    _zeros(br, "beta of the zero vector, lanc_run")
    seeds = [v0, z, _start2(e, 2)]
    ab, bb, nb = _batch(S, np.stack(seeds), NLONG, e)
    assert list(nb) == [NLONG, 0, NLONG]
    _zeros(ab[1], "alpha of the zero seed")
    _zeros(bb[1], "beta of the zero seed")
    _same(ab[0], a, "alpha seed 0")
    _same(bb[0], b, "beta seed 0")


def test_batch_equals_single_launches(launch):
    e, S, v0, (a, b, _) = launch
    seeds = [v0, _start2(e, 2), _start2(e, 3)]
    ab, bb, nb = _batch(S, np.stack(seeds), NLONG, e)
    for j, s in enumerate(seeds):
        a1, b1, n1 = S.lanc_tridiag(s, NLONG, real=not e.vc)
        assert nb[j] == n1 == NLONG
        _same(ab[j], a1, "alpha seed %d" % j)
        _same(bb[j], b1, "beta seed %d" % j)
    _same(ab[0], a, "alpha seed 0 against the fixture's run")


def test_continuation_launch(launch):
    """lanc_eigh runs launches of 64 steps: steps 65.. take the continuation
    path.  Its energy is a function of alpha / beta alone, so it equals the
    lowest eigenvalue of the tridiagonal of one launch of as many steps: two
    backward-stable eigensolvers, each off by O(n eps |T|) = 80 * 2.2e-16 |T|;
    the bar is 1e-12 |T|."""
    from scipy.linalg import eigvalsh_tridiagonal

    e, S, v0, _ = launch
    real = not e.vc
    e0, vec, ne = S.lanc_eigh(v0=v0, real=real, **pc.EIGH_KW)
    assert 64 < ne <= pc.EIGH_KW["nitermax"]
    a, b, ng = S.lanc_tridiag(v0, ne, real=real)     # one launch
    assert ng == ne
    t1 = eigvalsh_tridiagonal(a[:ne], b[1:ne])
    print(e.id, "continuation: |E0 - E0(one launch)| %.3e, |T| %.3f" % (abs(e0 - t1[0]), max(abs(t1[0]), abs(t1[-1]))))
    assert abs(e0 - t1[0]) <= 1e-12 * max(abs(t1[0]), abs(t1[-1]))
    assert abs(np.linalg.norm(vec) - 1.0) < 1e-10
    vc = np.asarray(vec, dtype=np.complex128)
    assert np.linalg.norm(S.hxv(vc) - e0 * vc) < 1e-5
