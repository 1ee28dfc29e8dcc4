"""How far a plain Lanczos run moves when only the summation order of its two dot products per step
changes: the one difference between ed_sector_lanc_tridiag_lockstep and the sequential runs.  CPU only
(numpy over the oracle's CSR and H·v): the figures behind STEPS = 8 and the two bars of
tests/test_gpu_lockstep.py, quoted in DESIGN.md §15.

  python tools/lockstep_dotorder.py

For c2 (4,4), hybrid (3,3) and replica_cplx (3,3) of tests/cases.py and six random seeds each: run A sums
conj(x)·y with numpy's pairwise sum; run B sums the same products in a random permutation of the rows, in
blocks of 256 added one after the other (the shape of a block reduction).  100 steps.  Printed: the largest
|alpha, beta difference| over the first 8 steps relative to max|alpha| + 2 max|beta|, and the largest
difference of the pole sums sum_j z_j^2 / (iw - (E_j - E_0)) on 32 Matsubara points at beta = 100, relative
to max|G|, E_0 the lowest Ritz value.  A manual tool: no test runs it.
"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dmft-ed_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import cases  # noqa: E402
from oracle.oracle import Oracle, spmv, spmv_real  # noqa: E402


def lanczos(csr, v0, n, dot, mv):
    r, p = v0.copy(), np.zeros_like(v0)
    b = np.sqrt(dot(r, r))
    A, B = [], [0.0]
    for _ in range(n):
        v = r / b
        w = mv(csr, v) - b * p
        a = dot(v, w)
        w = w - a * v
        p, r = v, w
        b = np.sqrt(dot(r, r))
        A.append(a)
        B.append(b)
    return np.array(A), np.array(B[:n])


def dot_pairwise(x, y):
    return float(np.sum((np.conj(x) * y).real))


def dot_permuted(perm):
    def dot(x, y):
        t = (np.conj(x) * y).real[perm]
        s = 0.0
        for i in range(0, len(t), 256):
            s += float(np.sum(t[i:i + 256]))
        return s
    return dot


def tridiag(a, b):
    return np.diag(a) + np.diag(b[1:], 1) + np.diag(b[1:], -1)


def pole_sum(a, b, wm, e0):
    E, Z = np.linalg.eigh(tridiag(a, b))
    return (Z[0] ** 2 / (1j * wm[:, None] - (E[None, :] - e0))).sum(1)


if __name__ == "__main__":
    wm = np.pi / 100 * (2 * np.arange(1, 33) - 1)
    for name, make, sec in (("c2", cases.c2, (4, 4)), ("hybrid", cases.hybrid, (3, 3)),
                            ("replica_cplx", cases.replica_cplx, (3, 3))):
        cfg = make()
        orc = Oracle(cfg)
        hmap = orc.build_sector(*sec)
        csr, dim, cplx = orc.build_csr(hmap), len(hmap), not cfg.is_real()
        mv = spmv if cplx else spmv_real
        rng = np.random.default_rng(1)
        w8 = wg = 0.0
        for _ in range(6):
            v0 = rng.normal(size=dim) + (1j * rng.normal(size=dim) if cplx else 0)
            n = min(100, dim)
            a1, b1 = lanczos(csr, v0, n, dot_pairwise, mv)
            a2, b2 = lanczos(csr, v0, n, dot_permuted(rng.permutation(dim)), mv)
            scale = np.max(np.abs(a1)) + 2 * np.max(np.abs(b1))
            w8 = max(w8, max(np.max(np.abs(a1[:8] - a2[:8])), np.max(np.abs(b1[:8] - b2[:8]))) / scale)
            e0 = np.linalg.eigvalsh(tridiag(a1, b1))[0]
            g1, g2 = pole_sum(a1, b1, wm, e0), pole_sum(a2, b2, wm, e0)
            wg = max(wg, np.max(np.abs(g1 - g2)) / np.max(np.abs(g1)))
        print(f"{name} {sec}, {dim} rows: first 8 steps {w8:.1e}, pole sums {wg:.1e}")
