"""Launch path of the persistent Lanczos kernel (csrc/ed_lanczos.hip,
csrc/ed_persist.hpp): a single run is one kernel on the stream (lanc_run) or
one kernel and the download of its LancState (lanc_tridiag, lanc_tridiag_dev,
lanc_eigh); the batched launch still downloads alpha, beta and the states.
The kernel reads a device start vector where it lies, initialises its
LancState and beta[0], stores alpha and beta of a single run straight into
the pinned staging block, and an early stop (breakdown, zero start vector)
writes the zeros behind its last step itself; no copy and no memset precede
the launch.  So stale alpha / beta of an earlier, longer run on the same
sector are what a mistake shows.

Shapes of tests/persist_mode4_cases.py where the launch path can go wrong:
nb3_2_2 (dim 36: idle lanes and padding slots), nb5_3_3 (dim 400), nb8_3_2
(the plain row loop, not software-pipelined).  Every comparison is bit for
bit: the runs compared execute the same kernel on the same numbers.

Early stop, case a (the converged ground vector of lanc_eigh, threshold
1e-13): a start vector stops the recurrence at its first step when its
residual |H v - E v| is below the threshold.  lanc_eigh stops on the energy,
|dE| <= 1e-13, which leaves a residual near sqrt(1e-13) (1.7e-7 on nb3_2_2),
so the test restarts lanc_eigh from its own Ritz vector until the vector
itself is converged (residuals 1.7e-7, 2.1e-12, 3.9e-15 on nb3_2_2: the run
from the third vector stops at step 1 with beta[1] = 3.5e-15).  It runs on
nb3_2_2 only: plain Lanczos without reorthogonalisation gets a Ritz vector
down to a residual of order eps |H| only in a sector this small.  Case b
(zero start vector) runs on all three shapes.

lanc_tridiag and the batch entry point mask everything past nlanc on the host,
so case a does not see the kernel's own zeros behind a breakdown.  lanc_run
returns the arrays unmasked but stops only below 1e-300, that is at a beta of
exactly 0: test_unmasked_breakdown takes a bath without hybridisation (H is
diagonal, every basis vector an exact eigenvector: w = H e_j - H_jj e_j = 0
in every bit) and checks the zeros behind step 1 of such a run after a longer
one.
"""
import numpy as np
import pytest

import persist_mode4_cases as pc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SHAPES = [c for c in pc.CASES if pc.key(c) in ("nb3_2_2", "nb5_3_3", "nb8_3_2")]
SHAPE_IDS = [pc.key(c) for c in SHAPES]


def _same(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    bad = np.nonzero(pc.bits(got) != pc.bits(want))[0]
    assert bad.size == 0, (what, "first differing entry", int(bad[0]), got[bad[0]], want[bad[0]])


def _zeros(x, what):
    # exactly +0.0, not merely == 0
    _same(x, np.zeros(np.shape(x)), what)


def _dev(v):
    t = torch.from_numpy(np.ascontiguousarray(v)).to("cuda:0").contiguous()
    torch.cuda.synchronize()
    return t


@pytest.fixture(scope="module", params=SHAPES, ids=SHAPE_IDS)
def shape(request):
    """One sector per shape with the runs every test compares against."""
    case = request.param
    with pc.open_sector(case) as S:
        assert S.lanc_mode(real=True) == 4
        n = pc.nsteps(S.dim)
        v0 = pc.start(S.dim)
        ref = S.lanc_tridiag(v0, n)
        assert ref[2] == n
        yield case, S, n, v0, ref


def test_lanc_run_matches_tridiag_and_leaves_start_vector(shape):
    case, S, n, v0, (a, b, _) = shape
    d = _dev(v0)
    before = d.clone()
    ar, br, _ = S.lanc_run(n, v0_dev=d)
    torch.cuda.synchronize()
    _same(ar, a, "alpha")
    _same(br, b, "beta")
    _zeros(br[:1], "beta[0]")
    assert torch.equal(d.view(torch.int64), before.view(torch.int64)), "start vector written"
    _same(d.cpu().numpy(), v0, "start vector")


def test_repeat_and_stale_data(shape):
    case, S, n, v0, (a, b, _) = shape
    d = _dev(v0)
    other = _dev(pc.start(S.dim, 2))
    r1 = S.lanc_run(n, v0_dev=d)
    r2 = S.lanc_run(n, v0_dev=d)
    _same(r2[0], r1[0], "alpha, second run")
    _same(r2[1], r1[1], "beta, second run")
    _same(r1[0], a, "alpha")
    # a run from another vector in between does not leak into the next
    ao, bo, _ = S.lanc_run(n, v0_dev=other)
    assert not np.array_equal(pc.bits(ao), pc.bits(a))
    m = min(10, n)
    short = S.lanc_run(m, v0_dev=d)
    _same(short[0], a[:m], "alpha, short run after a long one")
    _same(short[1], b[:m], "beta, short run after a long one")
    _same(S.lanc_run(n, v0_dev=other)[0], ao, "alpha, other vector again")
    r3 = S.lanc_run(n, v0_dev=d)
    _same(r3[0], a, "alpha, after the other vector")
    _same(r3[1], b, "beta, after the other vector")


def _batch(S, seeds_h, n, real=True):
    from edgpu.gf import _tridiag_batch

    return _tridiag_batch(S, _dev(np.stack(seeds_h)), n, real, 1e-13)


def test_zero_start_vector_after_a_longer_run(shape):
    case, S, n, v0, (a, b, _) = shape
    d = _dev(v0)
    S.lanc_run(n, v0_dev=d)                          # leaves n steps of alpha / beta behind
    z = np.zeros(S.dim)
    az, bz, nz = S.lanc_tridiag(z, n)
    assert nz == 0
    _zeros(az, "alpha of the zero vector")
    _zeros(bz, "beta of the zero vector")
    # lanc_run returns the device arrays unmasked: the kernel's own zeros
    S.lanc_run(n, v0_dev=d)
    ar, br, _ = S.lanc_run(n, v0_dev=_dev(z))
    _zeros(ar, "alpha of the zero vector, lanc_run")
    _zeros(br, "beta of the zero vector, lanc_run")
    # one such seed among normal ones
    seeds = [v0, z, pc.start(S.dim, 2)]
    ab, bb, nb = _batch(S, seeds, n)
    assert list(nb) == [n, 0, n]
    _zeros(ab[1], "alpha of the zero seed")
    _zeros(bb[1], "beta of the zero seed")
    _same(ab[0], a, "alpha seed 0")
    _same(bb[0], b, "beta seed 0")
    a2, b2, n2 = S.lanc_tridiag(seeds[2], n)
    assert n2 == n
    _same(ab[2], a2, "alpha seed 2")
    _same(bb[2], b2, "beta seed 2")


def test_breakdown_after_a_longer_run():
    """Case a: the run from the converged ground vector stops within a few
    steps; everything behind the stop is zero although a longer run came
    before it."""
    case = next(c for c in SHAPES if pc.key(c) == "nb3_2_2")
    with pc.open_sector(case) as S:
        assert S.lanc_mode(real=True) == 4
        n = pc.nsteps(S.dim)
        v0 = pc.start(S.dim)
        a, b, ng = S.lanc_tridiag(v0, n)             # the longer run
        assert ng == n
        # lanc_eigh stops on the energy (|dE| <= 1e-13), which leaves a residual
        # near sqrt(1e-13); restarted from its own Ritz vector it converges the
        # vector itself (each restart squares the error) until the run from it
        # breaks down at the threshold
        g = v0
        for restart in range(4):
            e0, g, ne = S.lanc_eigh(nitermax=S.dim, threshold=1e-13, v0=g, vector=True, real=True)
            g = np.ascontiguousarray(np.real(g), dtype=np.float64)
            ag, bg, nl = S.lanc_tridiag(g, n, threshold=1e-13)
            if nl <= 3:
                break
        assert 1 <= nl <= 3
        assert abs(ag[0] - e0) <= 1e-12 * abs(e0)
        _zeros(ag[nl:], "alpha past nlanc")
        _zeros(bg[nl + 1:], "beta past nlanc")
        _zeros(bg[:1], "beta[0]")
        # lanc_run (threshold 1e-300) does not stop on the same vector: no zero tail is expected of it,
        # only that the next stopping run is clean again
        S.lanc_run(n, v0_dev=_dev(v0))
        ag2, bg2, nl2 = S.lanc_tridiag(g, n, threshold=1e-13)
        assert nl2 == nl
        _same(ag2, ag, "alpha, stopping run repeated")
        _same(bg2, bg, "beta, stopping run repeated")
        seeds = [v0, g, pc.start(S.dim, 2)]
        ab, bb, nb = _batch(S, seeds, n)
        assert list(nb) == [n, nl, n]
        _same(ab[1], ag, "alpha of the stopping seed")
        _same(bb[1], bg, "beta of the stopping seed")
        _same(ab[0], a, "alpha seed 0")
        _same(bb[0], b, "beta seed 0")
        a2, b2, n2 = S.lanc_tridiag(seeds[2], n)
        _same(ab[2], a2, "alpha seed 2")
        _same(bb[2], b2, "beta seed 2")


def test_unmasked_breakdown():
    """beta = 0 exactly at step 1: lanc_run's unmasked alpha and beta are zero
    behind it although a full-length run on the same sector came before."""
    from edgpu.hamiltonian import Sector
    from edgpu.params import make_config

    cfg = make_config(Norb=1, Nbath=5)
    cfg.bath.v[...] = 0.0                            # no hybridisation: H diagonal
    with Sector(cfg, 3, 3, stored=True, real=True) as S:
        assert S.lanc_mode(real=True) >= 0           # a persistent mode takes the run
        n = pc.nsteps(S.dim)
        diag = np.real(S.hxv(np.ones(S.dim, dtype=np.complex128)))
        a, b, _ = S.lanc_run(n, v0_dev=_dev(pc.start(S.dim)))
        assert np.count_nonzero(a) > 1 and np.count_nonzero(b) > 1
        j = S.dim // 3
        e = np.zeros(S.dim)
        e[j] = 1.0
        ae, be, _ = S.lanc_run(n, v0_dev=_dev(e))
        _same(ae[:1], diag[j:j + 1], "alpha[0] = H_jj")
        _zeros(ae[1:], "alpha behind the breakdown")
        _zeros(be, "beta behind the breakdown")
        at, bt, nt = S.lanc_tridiag(e, n)
        assert nt == 1
        _same(at, ae, "alpha, masked entry point")
        _same(bt, be, "beta, masked entry point")


def test_complex_vectors_same_launch_path():
    case = next(c for c in SHAPES if pc.key(c) == "nb5_3_3")
    with pc.open_sector(case) as S:
        assert S.lanc_mode(real=False) >= 0          # a persistent mode takes the run
        n = pc.nsteps(S.dim)
        v0 = (pc.start(S.dim) + 1j * pc.start(S.dim, 3)).astype(np.complex128)
        a, b, ng = S.lanc_tridiag(v0, n, real=False)
        assert ng == n
        d = _dev(v0)
        before = d.clone()
        S.lanc_run(n, v0_dev=_dev(pc.start(S.dim, 2).astype(np.complex128)))
        ar, br, _ = S.lanc_run(n, v0_dev=d)
        torch.cuda.synchronize()
        _same(ar, a, "alpha")
        _same(br, b, "beta")
        _zeros(br[:1], "beta[0]")
        assert torch.equal(torch.view_as_real(d).view(torch.int64), torch.view_as_real(before).view(torch.int64))
