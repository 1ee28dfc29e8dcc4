"""Own rows of r_k in registers on the benchmark's shape of the persistent
MODE 4 Lanczos kernel (csrc/ed_persist.hpp): nb7_4_4, DimUp x DimDw = 70 x 70,
E = 4, RPT = 10.  That shape used to re-read its own rows from LDS; now the
kernel takes them from registers like the other real-vector shapes, so its
state in (start vector or saved r_k into registers and LDS), its state out
(r_k from registers) and the basis column changed path.  The recorded alpha
and beta of this shape are compared in tests/test_gpu_persist_mode4.py; here
are the launch-path cases of tests/test_gpu_persist_launch.py, which does not
run this shape: the zero start vector, a breakdown at step 1, the batched
launch, and continuation launches.  Every comparison is bit for bit: the runs
compared execute the same kernel on the same numbers.
"""
import numpy as np
import pytest

import persist_mode4_cases as pc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CASE = next(c for c in pc.CASES if pc.key(c) == "nb7_4_4")


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


@pytest.fixture(scope="module")
def sector():
    """The nb7_4_4 sector with the single run every test compares against."""
    with pc.open_sector(CASE) as S:
        assert (int(S.info.dimup), int(S.info.dimdw)) == CASE[2]
        assert pc.geometry(CASE[0], *CASE[1])[2:] == (4, 10)      # E, RPT
        assert S.lanc_mode(real=True) == 4
        n = pc.nsteps(S.dim)
        v0 = pc.start(S.dim)
        ref = S.lanc_tridiag(v0, n)
        assert ref[2] == n
        yield S, n, v0, ref


def test_zero_start_vector_after_a_longer_run(sector):
    S, n, v0, (a, b, _) = sector
    d = _dev(v0)
    ar, br, _ = S.lanc_run(n, v0_dev=d)              # leaves n steps of alpha / beta behind
    _same(ar, a, "alpha")
    _same(br, b, "beta")
    z = np.zeros(S.dim)
    az, bz, nz = S.lanc_tridiag(z, n)
    assert nz == 0                                   # iter 0, done set
    _zeros(az, "alpha of the zero vector")
    _zeros(bz, "beta of the zero vector")
    # lanc_run returns the arrays unmasked: the kernel's own zeros
    S.lanc_run(n, v0_dev=d)
    ar, br, _ = S.lanc_run(n, v0_dev=_dev(z))
    _zeros(ar, "alpha of the zero vector, lanc_run")
    _zeros(br, "beta of the zero vector, lanc_run")
    # the run after it is the recorded one again
    ar, br, _ = S.lanc_run(n, v0_dev=d)
    _same(ar, a, "alpha after the zero vector")
    _same(br, b, "beta after the zero vector")


def test_unmasked_breakdown():
    """Bath without hybridisation: H is diagonal, every basis vector an exact
    eigenvector (w = H e_j - H_jj e_j = 0 in every bit), so the run stops at
    step 1 with beta = 0 exactly; lanc_run's unmasked alpha and beta are +0.0
    behind it although a full-length run on the same sector came before."""
    from edgpu.hamiltonian import Sector
    from edgpu.params import make_config

    cfg = make_config(Norb=1, Nbath=CASE[0])
    cfg.bath.v[...] = 0.0
    with Sector(cfg, CASE[1][0], CASE[1][1], stored=True, real=True) as S:
        assert (int(S.info.dimup), int(S.info.dimdw)) == CASE[2]
        assert S.lanc_mode(real=True) == 4
        n = pc.nsteps(S.dim)
        diag = np.real(S.hxv(np.ones(S.dim, dtype=np.complex128)))
        a, b, _ = S.lanc_run(n, v0_dev=_dev(pc.start(S.dim)))
        assert np.count_nonzero(a) > 1 and np.count_nonzero(b) > 1
        # a row of the last slot (r = 9) and one of the first
        for j in (S.dim - 3, 5):
            e = np.zeros(S.dim)
            e[j] = 1.0
            S.lanc_run(n, v0_dev=_dev(pc.start(S.dim)))
            ae, be, _ = S.lanc_run(n, v0_dev=_dev(e))
            _same(ae[:1], diag[j:j + 1], "alpha[0] = H_jj")
            _zeros(ae[1:], "alpha behind the breakdown")
            _zeros(be, "beta behind the breakdown")
            at, bt, nt = S.lanc_tridiag(e, n)
            assert nt == 1
            _same(at, ae, "alpha, masked entry point")
            _same(bt, be, "beta, masked entry point")


def test_batched_launch_equals_single_runs(sector):
    """One workgroup per start vector: state in and out of the batch from
    registers; every run equals its single lanc_tridiag run."""
    from edgpu.gf import _tridiag_batch

    S, n, v0, (a, b, _) = sector
    seeds_h = np.stack([pc.start(S.dim, j + 1) for j in range(pc.NBATCH)])
    assert pc.NBATCH == 3
    ab, bb, nb = _tridiag_batch(S, _dev(seeds_h), n, True, 1e-13)
    for j in range(pc.NBATCH):
        aj, bj, nj = S.lanc_tridiag(seeds_h[j], n)
        assert nb[j] == nj == n
        _same(ab[j], aj, "alpha seed %d" % j)
        _same(bb[j], bj, "beta seed %d" % j)
    _same(ab[0], a, "alpha seed 0, the module's run")
    _same(bb[0], b, "beta seed 0, the module's run")


def test_continuation_launches_repeat(sector):
    """lanc_eigh in launches of 64 steps: steps 65.. reload r_k and p from
    memory into registers (first = 0) after the first launch stored them from
    registers.  Twice from the same vector: identical bits; as many steps as
    the one-launch tridiagonal of that length."""
    S, n, v0, _ = sector
    e1, vec1, ne1 = S.lanc_eigh(v0=v0, **pc.EIGH_KW)
    S.lanc_run(n, v0_dev=_dev(pc.start(S.dim, 2)))   # another run in between
    e2, vec2, ne2 = S.lanc_eigh(v0=v0, **pc.EIGH_KW)
    assert 64 < ne1 <= pc.EIGH_KW["nitermax"]
    assert ne2 == ne1
    _same([e2], [e1], "E0")
    _same(np.real(vec2), np.real(vec1), "Ritz vector, real part")
    _same(np.imag(vec2), np.imag(vec1), "Ritz vector, imaginary part")
    at, bt, nt = S.lanc_tridiag(v0, ne1)             # one launch
    assert nt == ne1
