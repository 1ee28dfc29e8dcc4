"""ed_sector_twin_vector (k_twin_transpose, k_twin_gather) on the MI355X.

Contract (es_return_cvector of a twin entry, ED_EIGENSPACE.f90:414-445, with
twin_sector_order / flip_state, ED_SETUP.f90:1123-1186):
dst_vec[i] = src_vec[argsort(flip_state(map_src))[i]].  The kernels only move
values, so every comparison with numpy is bit for bit.
"""
import ctypes

import numpy as np
import pytest

import cases
from edgpu import _lib
from edgpu.hamiltonian import Sector
from edgpu.params import make_config

pytestmark = pytest.mark.gpu

NS9 = lambda: make_config(Norb=1, Nbath=8)     # noqa: E731  (Ns = 9: C(9,k) = 1, 9, 36, 84, 126)
# (config, src sector, dst sector): DimUp x DimDw of src in the comments
NORMAL = [(NS9, (3, 5), (5, 3)),        # 84 x 126: ragged tiles in both directions
          (NS9, (4, 5), (5, 4)),        # 126 x 126: 4 x 4 tiles, the last ones partial
          (NS9, (1, 4), (4, 1)),        # 9 x 126: one partial tile across
          (NS9, (0, 3), (3, 0)),        # 1 x 84: a single column
          (NS9, (3, 0), (0, 3)),        # 84 x 1: a single row
          (NS9, (9, 0), (0, 9)),        # dim 1
          (cases.c2, (4, 4), (4, 4))]   # 70 x 70: a sector that is its own twin


def _flip(cfg, states):
    s = states.astype(np.int64)
    Ns = cfg.Ns
    if cfg.ed_mode == "nonsu2":
        return ~s & ((1 << (2 * Ns)) - 1)
    return ((s & ((1 << Ns) - 1)) << Ns) | (s >> Ns)


def _open(cfg, q, **kw):
    return Sector(cfg, q[0], q[1], stored=False, direct=True, real=cfg.is_real(), **kw)


def _vectors(dim, seed):
    rng = np.random.default_rng(seed)
    return [rng.normal(size=dim), rng.normal(size=dim) + 1j * rng.normal(size=dim)]


@pytest.mark.parametrize("mk,qa,qb", NORMAL, ids=[f"{a}->{b}" for _, a, b in NORMAL])
def test_normal_mode_transpose_and_gather_match_argsort(mk, qa, qb):
    cfg = mk()
    with _open(cfg, qa) as A, _open(cfg, qb) as B, _open(cfg, qb, options=("twin_gather",)) as Bg:
        order = np.argsort(_flip(cfg, A.map()), kind="stable")
        assert np.array_equal(_flip(cfg, A.map())[order], B.map().astype(np.int64))   # dst really is the twin
        up, dw = int(A.info.dimup), int(A.info.dimdw)
        assert np.array_equal(order, np.arange(A.dim).reshape(dw, up).T.reshape(-1))   # the transpose
        for x in _vectors(A.dim, A.dim):
            t = A.twin_vector(B, x).cpu().numpy()
            g = A.twin_vector(Bg, x).cpu().numpy()
            assert t.dtype == x.dtype and np.array_equal(t, x[order]) and np.array_equal(g, t)


@pytest.mark.parametrize("name,qa,qb", [("superc", (1, 0), (-1, 0)), ("nonsu2_rand", (5, 0), (7, 0))])
def test_generic_kernel_superc_and_nonsu2(name, qa, qb):
    cfg = dict((c[0], c[1]) for c in cases.CASES)[name]()
    with _open(cfg, qa) as A, _open(cfg, qb) as B:
        order = np.argsort(_flip(cfg, A.map()), kind="stable")
        assert np.array_equal(_flip(cfg, A.map())[order], B.map().astype(np.int64))
        for x in _vectors(A.dim, 5):
            t = A.twin_vector(B, x).cpu().numpy()
            assert np.array_equal(t, x[order])
            if name == "nonsu2_rand":                 # complementing all bits reverses the order
                assert np.array_equal(t, x[::-1])
        # there and back again: the twin map is an involution
        x = _vectors(A.dim, 6)[1]
        assert np.array_equal(B.twin_vector(A, A.twin_vector(B, x)).cpu().numpy(), x)


def _rc(A, B, x, y):
    import torch

    torch.cuda.synchronize()
    rc = _lib.load().ed_sector_twin_vector(A.handle, B.handle, 0, ctypes.c_void_p(x.data_ptr()),
                                           ctypes.c_void_p(y.data_ptr()), None)
    torch.cuda.synchronize()
    return rc


def test_refusals_leave_dst_untouched():
    """ED_ERR_ARG = 1 before any launch: dst not the twin, a Jz_basis sector,
    sectors of two different models; ED_ERR_UNSUPPORTED = 5 for a row split."""
    import torch

    cfg = NS9()
    dev = torch.device("cuda", 0)

    def attempt(A, B, want):
        x = torch.ones(A.dim, dtype=torch.float64, device=dev)
        y = torch.full((max(A.dim, B.dim),), 7.0, dtype=torch.float64, device=dev)
        assert _rc(A, B, x, y) == want
        assert bool(torch.all(y == 7.0))
        assert _rc(A, B, x, x) == 1                            # aliased vectors

    with _open(cfg, (3, 5)) as A, _open(cfg, (3, 5)) as same, _open(cfg, (5, 4)) as other:
        attempt(A, same, 1)
        attempt(A, other, 1)
        with pytest.raises(_lib.EDGPUError, match="ED_ERR_ARG"):
            A.twin_vector(other, np.ones(A.dim))
        with _open(make_config(Norb=1, Nbath=7), (5, 3)) as B8:           # Ns = 8: another model
            attempt(A, B8, 1)
        with _open(make_config(Norb=1, Nbath=8, Nspin=2, ed_mode="nonsu2"), (10, 0)) as Bn:
            attempt(A, Bn, 1)
        with Sector(cfg, 5, 3, stored=True, real=True, rows=(0, 100)) as Brow:
            attempt(A, Brow, 5)
    jz = cases.nonsu2_jz()
    with _open(jz, (5, 1)) as A, _open(jz, (7, -3)) as B:
        attempt(A, B, 1)
        with pytest.raises(_lib.EDGPUError, match="Jz"):
            A.twin_vector(B, np.ones(A.dim, dtype=np.complex128))


def test_twin_commutes_with_the_hamiltonian():
    """c2 is spin symmetric: H_(5,3) twin(x) = twin(H_(3,5) x), within 1e-13
    of each row's sum_j |H_ij x_j| (the two sides add the same terms in
    another order: the project's bar for reordered row sums)."""
    import torch

    cfg = cases.c2()
    with Sector(cfg, 3, 5, stored=True, real=True) as A, Sector(cfg, 5, 3, stored=True, real=True) as B:
        dev = torch.device("cuda", 0)
        x = torch.from_numpy(np.random.default_rng(35).normal(size=A.dim)).to(dev)
        hx, tx = torch.empty_like(x), A.twin_vector(B, x)
        A.hxv_dev(x, hx)
        htx = torch.empty_like(tx)
        B.hxv_dev(tx, htx)
        torch.cuda.synchronize()
        lhs, rhs = htx.cpu().numpy(), A.twin_vector(B, hx).cpu().numpy()
        rp, cols, vals = B.dump_csr()
        txh = tx.cpu().numpy()
        rows = np.repeat(np.arange(B.dim), np.diff(rp))
        scale = np.zeros(B.dim)
        np.add.at(scale, rows, np.abs(vals) * np.abs(txh[cols]))
        ratio = np.max(np.abs(lhs - rhs) / scale)
        print(f"max |H twin(x) - twin(H x)| / sum|H_ij x_j| = {ratio:.3e}")
        assert ratio < 1e-13
