"""Persistent MODE 4 Lanczos kernel, real vectors (csrc/ed_persist.hpp): every
code shape of the Kronecker register layout against the multi-kernel
recurrence, and bit for bit against alpha/beta recorded from the build before
the kernel's step was trimmed (tests/golden/persist_mode4_parent.npz, written
by tests/golden/make_persist_mode4_parent.py).  The trims remove register
moves, a second read and product of the own rows, and move loads: a
floating-point operation that changed, or changed place, shows as a differing
bit.

Against the multi-kernel recurrence: the first 40 steps at rtol 1e-9, atol
1e-11 (the bars of test_gpu_lanczos.test_persistent_matches_multikernel).  The
two differ in summation order, and an unreorthogonalised recurrence amplifies
that once Ritz values converge, which a sector of dimension n reaches well
before n steps; the 36-dimensional sector is therefore compared over its first
dim // 2 = 18 steps (recorded on the build before the change: its two
recurrences part by more than 1e-9 at step 27, the larger sectors' at step 50
or later).  The comparison with the fixture covers every step of every sector.
"""
import os

import numpy as np
import pytest

import persist_mode4_cases as pc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "persist_mode4_parent.npz")


@pytest.fixture(scope="module")
def parent():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def _assert_bits(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    assert np.array_equal(pc.bits(got), pc.bits(want)), (
        what, "first differing step", int(np.nonzero(pc.bits(got) != pc.bits(want))[0][0]))


@pytest.mark.parametrize("case", pc.CASES, ids=pc.IDS)
def test_shape_matches_multikernel_and_parent(case, parent):
    k = pc.key(case)
    with pc.open_sector(case) as S:
        geo = pc.geometry(case[0], *case[1])
        assert (int(S.info.dimup), int(S.info.dimdw)) == geo[:2] == case[2]
        assert geo[2:] == case[3:5]                      # E, RPT of pkr_geom
        assert (geo[2] * geo[3] <= 40) == case[5]        # the software-pipelined row loop, or not
        assert S.lanc_mode(real=True) == 4
        n = pc.nsteps(S.dim)
        v0 = pc.start(S.dim)
        a, b, ng = S.lanc_tridiag(v0, n)
        S.set_options("no_persist")
        a2, b2, n2 = S.lanc_tridiag(v0, n)
    assert ng == n2 == n
    m = min(40, S.dim // 2)
    np.testing.assert_allclose(a[:m], a2[:m], rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(b[:m], b2[:m], rtol=1e-9, atol=1e-11)
    assert ng == int(parent["n_" + k])
    _assert_bits(a, parent["a_" + k], "alpha " + k)
    _assert_bits(b, parent["b_" + k], "beta " + k)


@pytest.mark.parametrize("case", pc.LEG_CASES, ids=pc.LEG_IDS)
def test_continuation_launches_and_kept_basis(case, parent):
    """lanc_eigh with the Krylov basis kept: launches of 64 steps, so steps
    65.. run the continuation path (first = 0, R and P reloaded) and every
    step stores its basis column.  The energy is a function of alpha/beta
    alone (host tql2): equal bits with the recorded build's, and equal to the
    lowest eigenvalue of the tridiagonal of ONE launch of as many steps
    (lanc_tridiag and the batch entry point run any length in one launch, so
    alpha/beta of a split run are not returned anywhere: the energy stands
    for them).  Ritz vector as in test_tridiag_and_ground_state."""
    from scipy.linalg import eigvalsh_tridiagonal

    k = pc.key(case)
    with pc.open_sector(case) as S:
        assert S.lanc_mode(real=True) == 4
        v0 = pc.start(S.dim)
        e0, vec, ne = S.lanc_eigh(v0=v0, **pc.EIGH_KW)
        assert 64 < ne <= pc.EIGH_KW["nitermax"]
        a, b, ng = S.lanc_tridiag(v0, ne)                # one launch
        res = np.linalg.norm(S.hxv(vec.astype(np.complex128)) - e0 * vec)
    assert ng == ne == int(parent["ne_" + k])
    _assert_bits([e0], [parent["e0_" + k]], "E0 " + k)
    # the one-launch run's first 60 steps are the recorded ones
    _assert_bits(a[:pc.NSTEP], parent["a_" + k], "alpha " + k)
    _assert_bits(b[:pc.NSTEP], parent["b_" + k], "beta " + k)
    # same tridiagonal, two backward-stable symmetric eigensolvers: each off by
    # O(n eps |T|) = 80 * 2.2e-16 * |T|; bar 1e-12 |T| (> 50 times that)
    t1 = eigvalsh_tridiagonal(a[:ne], b[1:ne])
    assert abs(e0 - t1[0]) <= 1e-12 * max(abs(t1[0]), abs(t1[-1]))
    assert abs(np.linalg.norm(vec) - 1.0) < 1e-10
    assert res < 1e-5


@pytest.mark.parametrize("case", pc.LEG_CASES, ids=pc.LEG_IDS)
def test_batched_launch(case, parent):
    """One workgroup per start vector: every run equals its single launch,
    run 0 (v0 = sin(1..dim)) the recorded one."""
    from edgpu.gf import _tridiag_batch

    k = pc.key(case)
    with pc.open_sector(case) as S:
        assert S.lanc_mode(real=True) == 4
        n = pc.nsteps(S.dim)
        seeds_h = np.stack([pc.start(S.dim, j + 1) for j in range(pc.NBATCH)])
        seeds = torch.from_numpy(seeds_h).to("cuda:0").contiguous()
        torch.cuda.synchronize()
        ab, bb, nb = _tridiag_batch(S, seeds, n, True, 1e-13)
        single = [S.lanc_tridiag(seeds_h[j], n) for j in range(pc.NBATCH)]
    for j in range(pc.NBATCH):
        assert nb[j] == single[j][2] == n
        _assert_bits(ab[j], single[j][0], "alpha seed %d" % j)
        _assert_bits(bb[j], single[j][1], "beta seed %d" % j)
    _assert_bits(ab[0], parent["a_" + k], "alpha " + k)
    _assert_bits(bb[0], parent["b_" + k], "beta " + k)
