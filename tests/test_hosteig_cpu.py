"""The host half of the Lanczos solvers (dmft-ed_amd/csrc/ed_hosteig.hpp) on
the CPU: no GPU, no HIP.  A stand-alone C++ driver (its own main, written and
compiled here with plain g++) reads cases from a file and prints results as
hex floats, so every comparison below is on exact bits.

Checked: the implicit-QL routine in its three rotation modes against each
other, the oracle's tql2 (EISPACK pythag) and LAPACK (hypot variant); the
restart's dense eigen-solver sym_eigh and its fallback jacobi_eigh; the
restart-cycle decisions (projected matrix, breakdown column, ARPACK count,
nkeep, arrowhead) against their formulas restated in numpy; and the
degeneracy screen's decision on one tridiagonal per outcome.
"""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dmft-ed_amd", "csrc")

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "ed_hosteig.hpp"
using namespace edg;
static FILE* in;
static std::string tok() {
  char b[128];
  if (fscanf(in, "%127s", b) != 1) return "";
  return b;
}
static long I() { return strtol(tok().c_str(), nullptr, 10); }
static double D() { return strtod(tok().c_str(), nullptr); }
static std::vector<double> A(size_t n) {
  std::vector<double> v(n);
  for (auto& x : v) x = D();
  return v;
}
static void out(const double* p, size_t n) {
  for (size_t i = 0; i < n; i++) printf(" %a", p[i]);
}
template <bool FAST>
static void ql(int mode, int n, std::vector<double> d, std::vector<double> e) {
  // mode 0: no Z; 1: full Z from the identity; 2: first row only
  std::vector<double> z((size_t)n * n, 0.0), row(n, 0.0);
  int rc = 0;
  if (mode == 0) {
    rc = tql2<FAST>(n, d.data(), e.data(), nullptr);
  } else if (mode == 1) {
    for (int i = 0; i < n; i++) z[i + (size_t)n * i] = 1.0;
    rc = tql2<FAST>(n, d.data(), e.data(), z.data());
    for (int i = 0; i < n; i++) row[i] = z[(size_t)n * i];
  } else if (!FAST) {
    std::vector<double> E(n), z2(n);
    rc = tridiag_poles(n, d.data(), e.data(), E.data(), z2.data(), row.data());
    d = E;
  } else {
    for (int i = 0; i + 1 < n; i++) e[i] = e[i + 1];
    e[n - 1] = 0.0;
    row[0] = 1.0;
    rc = ql_implicit<true>(n, d.data(), e.data(), QlRowZ{row.data()});
  }
  printf("%d", rc);
  out(d.data(), n);
  out(row.data(), n);
  printf("\n");
}
int main(int argc, char** argv) {
  in = argc > 1 ? fopen(argv[1], "r") : stdin;
  if (!in) return 2;
  for (std::string c = tok(); !c.empty(); c = tok()) {
    if (c == "ql") {
      const int fast = I(), mode = I(), n = I();
      auto d = A(n), e = A(n);
      if (fast) ql<true>(mode, n, d, e);
      else ql<false>(mode, n, d, e);
    } else if (c == "eigh") {
      const int jac = I(), n = I();
      auto a = A((size_t)n * n);
      std::vector<double> w, Z;
      if (jac) jacobi_eigh(n, a, w, Z);
      else sym_eigh(n, a, w, Z);
      printf("0");
      out(w.data(), n);
      out(Z.data(), (size_t)n * n);
      printf("\n");
    } else if (c == "fill") {
      const int ma = I(), k0 = I(), j0 = I(), m = I();
      auto al = A(m), be = A(m), Tm = A((size_t)ma * ma);
      printf("%d", trl_fill(Tm.data(), ma, k0, j0, m, al.data(), be.data()));
      out(Tm.data(), Tm.size());
      printf("\n");
    } else if (c == "nconv") {
      const int ma = I(), nev = I();
      const double beta = D(), tol = D();
      auto th = A(ma), Z = A((size_t)ma * ma);
      printf("%d\n", trl_nconv(ma, nev, beta, th.data(), Z.data(), tol));
    } else if (c == "nkeep") {
      const int ma = I(), nev = I();
      printf("%d\n", trl_nkeep(ma, nev));
    } else if (c == "arrow") {
      const int ma = I(), nkeep = I();
      const double beta = D();
      auto th = A(ma), Z = A((size_t)ma * ma), Tm = A((size_t)ma * ma);
      trl_arrowhead(Tm.data(), ma, nkeep, beta, th.data(), Z.data());
      printf("0");
      out(Tm.data(), Tm.size());
      printf("\n");
    } else if (c == "screen") {
      const int K = I();
      const double cut = D(), tol = D();
      auto al = A(K), be = A(K);
      printf("%d\n", (int)screen_decide(al, be, cut, tol));
    } else if (c == "setup") {
      const int m = I(), nev = I();
      const long dim = I();
      const int opts = I(), conv = I();
      const double evtop = D(), tol = D();
      const ScreenPlan p = screen_setup(m, nev, dim, opts, conv, evtop, tol);
      printf("%d %a %a %a %a %a\n", p.mp, (double)p.verify, (double)p.hint, p.cut, p.tprobe, (double)p.maxsteps);
    } else {
      return 3;
    }
  }
  return 0;
}
"""


def _build(dirpath, extra=()):
    src = dirpath / "hosteig_driver.cpp"
    src.write_text(DRIVER)
    exe = dirpath / ("hosteig_driver" + ("_san" if extra else ""))
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", *extra, "-I", CSRC, str(src), "-o", str(exe)],
                   check=True)
    return str(exe)


def _hx(a):
    return " ".join(float(x).hex() for x in np.asarray(a, dtype=np.float64).ravel(order="F"))


class Driver:
    """Collects cases, runs the driver once, hands out the parsed result lines."""

    def __init__(self):
        self.lines = []
        self.results = None

    def add(self, *parts):
        self.lines.append(" ".join(str(p) if isinstance(p, (int, str)) else _hx(p) for p in parts))
        return len(self.lines) - 1

    def run(self, exe, path):
        path.write_text("\n".join(self.lines) + "\n")
        out = subprocess.run([exe, str(path)], capture_output=True, text=True, check=True).stdout
        rows = out.strip().split("\n")
        assert len(rows) == len(self.lines)
        self.raw = out
        self.results = [(int(r.split()[0]), np.array([float.fromhex(t) for t in r.split()[1:]])) for r in rows]


# ------------------------------------------------------------------ cases
def _tridiagonals():
    rng = np.random.default_rng(20240611)
    out = []
    for n in (1, 2, 5, 23, 64):
        out.append((rng.normal(size=n), np.concatenate([[0.0], np.abs(rng.normal(size=n - 1))])))
    out.append((np.array([1.0, -2.0, 0.5, 3.0]), np.array([0.0, 0.7, 0.0, 0.2])))  # split
    return out


def _arrowhead_case(rng, n=23, nkeep=14):
    """The projected matrix after a restart and the next sweep: kept Ritz
    values on the diagonal, the residual's couplings in row/column nkeep, the
    new Lanczos steps as a tridiagonal tail."""
    A = np.zeros((n, n))
    A[np.arange(nkeep), np.arange(nkeep)] = np.sort(rng.normal(size=nkeep))
    A[nkeep, :nkeep] = A[:nkeep, nkeep] = 1e-3 * rng.normal(size=nkeep)
    for j in range(nkeep, n):
        A[j, j] = rng.normal()
        if j + 1 < n:
            A[j, j + 1] = A[j + 1, j] = abs(rng.normal())
    return A


def _dense_cases():
    rng = np.random.default_rng(77)
    mats = []
    for n in (2, 3, 23, 32):
        B = rng.normal(size=(n, n))
        mats.append((B + B.T) / 2)
    mats.append(_arrowhead_case(rng))
    return mats


M, NEV = 23, 6
BREAK_REL, EPS23 = 1e-13, 3.6e-11   # the constants of the rules restated below


def _fill_ref(Tm, k0, j0, al, be):
    """trlan_core's fill of the projected matrix and its breakdown test."""
    ma = M - k0
    T = Tm.copy()
    for j in range(j0, M):
        l = j - k0
        T[l, l] = al[j]
        if l + 1 < ma:
            T[l, l + 1] = T[l + 1, l] = be[j]
        scale = abs(al[j]) + (abs(T[l - 1, l]) if l > 0 else 0.0) + 1e-300
        if l + 1 < ma and be[j] < BREAK_REL * scale:
            return j, T
    return -1, T


def _nkeep_ref(ma, nev):
    return max(nev, min(ma - 2, nev + (ma - nev) // 2))


def _restart_cases():
    """(k0, j0, al, be, Tm_in, label): a first sweep and a sweep after a
    restart for k0 = 0 and k0 = 6, each with and without a broken-down beta."""
    rng = np.random.default_rng(5)
    cases = []
    for k0 in (0, 6):
        ma = M - k0
        nkeep = _nkeep_ref(ma, NEV if k0 == 0 else 1)
        for j0 in (k0, k0 + nkeep):
            for broken in (False, True):
                al = rng.normal(size=M)
                be = 0.3 + np.abs(rng.normal(size=M))
                Tm = np.zeros((ma, ma))
                if j0 > k0:  # the arrowhead a restart left
                    Tm[np.arange(nkeep), np.arange(nkeep)] = np.sort(rng.normal(size=nkeep))
                    Tm[nkeep, :nkeep] = Tm[:nkeep, nkeep] = 1e-2 * rng.normal(size=nkeep)
                if broken:  # just under 1e-13 * scale at one column, just over it at an earlier one
                    jb = j0 + 3
                    scale = abs(al[jb]) + be[jb - 1]
                    be[jb] = 0.9 * BREAK_REL * scale
                    be[j0 + 1] = 1.1 * BREAK_REL * (abs(al[j0 + 1]) + be[j0])
                cases.append((k0, j0, al, be, Tm, broken))
    return cases


def _lanczos(diag, v, K):
    """Plain Lanczos with full reorthogonalisation on a diagonal matrix:
    al[k], be[k] = |w_k| (the screen's convention: be[K-1] is the residual)."""
    V = [v / np.linalg.norm(v)]
    al, be = [], []
    for k in range(K):
        w = diag * V[k]
        al.append(V[k] @ w)
        for _ in range(2):
            for u in V:
                w = w - (u @ w) * u
        be.append(np.linalg.norm(w))
        V.append(w / be[-1])
    return np.array(al), np.array(be)


def _ritz(al, be):
    """Lowest Ritz value and its residual bound, as tests/test_screen_rule.py."""
    T = np.diag(al) + np.diag(be[:-1], 1) + np.diag(be[:-1], -1)
    e, Z = np.linalg.eigh(T)
    return e[0], abs(be[-1] * Z[-1, 0])


SCREEN_TOL = 1e-5   # the probe's screen tolerance (kProbeTol)
BELOW, NONE, UNDECIDED = 1, 0, -1


def _screen_cases():
    """(label, al, be, cut, expected) with the premises of each case asserted
    here on the numpy restatement of the rule."""
    rng = np.random.default_rng(11)
    n = 400
    spec = np.concatenate([[-3.0], np.linspace(-1.0, 2.0, n - 1)])
    v = rng.uniform(-1, 1, n)
    out = []

    def premises(al, be, cut):
        th, r = _ritz(al, be)
        inv = be[-1] < BREAK_REL * (abs(th) + 1e-300)
        conv = r <= SCREEN_TOL * max(EPS23, abs(th))
        return th, r, inv, conv

    # the lowest Ritz value converged, residual norm not small: K = 40
    al, be = _lanczos(spec, v, 40)
    th, r = _ritz(al, be)
    # below
    cut = th + 1e-9
    assert th < cut
    out.append(("below", al, be, cut, BELOW))
    # none by convergence, the whole residual interval above the cut
    cut = th - 1e-3
    _, _, inv, conv = premises(al, be, cut)
    assert not inv and conv and th - r > cut
    out.append(("none-converged", al, be, cut, NONE))
    # undecided: theta far above the cut but not converged (K = 6)
    al6, be6 = _lanczos(spec, v, 6)
    th6, r6 = _ritz(al6, be6)
    cut = th6 - 1.0
    _, _, inv, conv = premises(al6, be6, cut)
    assert not inv and not conv and th6 - r6 > cut
    out.append(("undecided", al6, be6, cut, UNDECIDED))
    # adversarial (the comment above probe_screen): a well-converged theta
    # just above the cut whose residual interval reaches below it
    for K in range(8, 40):
        alK, beK = _lanczos(spec, v, K)
        thK, rK = _ritz(alK, beK)
        if 1e-9 * abs(thK) < rK <= 0.1 * SCREEN_TOL * abs(thK):
            break
    cut = thK - 0.5 * rK
    _, _, inv, conv = premises(alK, beK, cut)
    assert not inv and conv and thK > cut + 1e-12 and not thK - rK > cut
    out.append(("adversarial", alK, beK, cut, UNDECIDED))
    # none by invariance alone: beta_K under 1e-13 |theta| with the lowest
    # Ritz vector sitting on the last Krylov vector, and the cut inside the
    # (tiny) residual interval so that the convergence rule cannot answer
    ali = np.array([0.5, 1.0, 0.0, -5.0])
    bei = np.array([0.4, 0.3, 1e-3, 0.0])
    bei[-1] = 0.9 * BREAK_REL * 5.0
    thi, ri = _ritz(ali, bei)
    cut = thi - 0.5 * ri
    _, _, inv, conv = premises(ali, bei, cut)
    assert inv and conv and thi > cut and not thi - ri > cut
    assert 0.5 * ri > 100 * np.spacing(abs(thi))   # the window is wide against rounding in theta
    out.append(("none-invariant", ali, bei, cut, NONE))
    return out


# ------------------------------------------------------------------ fixture
@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = tmp_path_factory.mktemp("hosteig")
    drv = Driver()
    ids = {}
    for t, (a, b) in enumerate(_tridiagonals()):
        for fast in (0, 1):
            for mode in (0, 1, 2):
                ids["ql", t, fast, mode] = drv.add("ql", fast, mode, len(a), a, b)
    for t, A in enumerate(_dense_cases()):
        for jac in (0, 1):
            ids["eigh", t, jac] = drv.add("eigh", jac, len(A), A)
    for t, (k0, j0, al, be, Tm, _) in enumerate(_restart_cases()):
        ids["fill", t] = drv.add("fill", M - k0, k0, j0, M, al, be, Tm)
    for t, (_, al, be, cut, _) in enumerate(_screen_cases()):
        ids["screen", t] = drv.add("screen", len(al), [cut], [SCREEN_TOL], al, be)
    drv.ids = ids
    drv.dir = d
    drv.exe = _build(d)
    drv.run(drv.exe, d / "cases.txt")
    return drv


def _split(res, n):
    return res[:n], res[n:]


# -------------------------------------------------------------------- tests
def test_ql_modes_bit_identical_and_match_oracle(run):
    from scipy.linalg import eigh_tridiagonal

    from oracle.oracle import tql2

    for t, (a, b) in enumerate(_tridiagonals()):
        n = len(a)
        for fast in (0, 1):
            rc0, r0 = run.results[run.ids["ql", t, fast, 0]]
            rc1, r1 = run.results[run.ids["ql", t, fast, 1]]
            rc2, r2 = run.results[run.ids["ql", t, fast, 2]]
            assert rc0 == rc1 == rc2 == 0
            d0, _ = _split(r0, n)
            d1, z1 = _split(r1, n)
            d2, z2 = _split(r2, n)
            np.testing.assert_array_equal(d0, d1)
            np.testing.assert_array_equal(d1, d2)
            np.testing.assert_array_equal(z1, z2)
            assert np.all(np.diff(d1) >= 0)
            if n == 1:
                assert d1[0] == a[0] and z2[0] == 1.0
                continue
            if not fast:  # EISPACK pythag: the oracle's tql2, bit for bit
                W, Z, ierr = tql2(a.copy(), b.copy())
                assert ierr == 0
                np.testing.assert_array_equal(d1, W)
                np.testing.assert_array_equal(z1, Z[0])
            else:
                w, z = eigh_tridiagonal(a, b[1:], lapack_driver="stev")
                np.testing.assert_allclose(d1, w, rtol=0, atol=1e-12)
                np.testing.assert_allclose(z1 ** 2, z[0] ** 2, rtol=0, atol=1e-12)


@pytest.mark.parametrize("jac", [0, 1], ids=["sym_eigh", "jacobi_eigh"])
def test_dense_eigh(run, jac):
    for t, A in enumerate(_dense_cases()):
        n = len(A)
        rc, r = run.results[run.ids["eigh", t, jac]]
        w, z = _split(r, n)
        Z = z.reshape(n, n, order="F")
        wref = np.linalg.eigh(A)[0]
        assert np.all(np.diff(w) >= 0)
        assert np.max(np.abs(w - wref)) <= 1e-12 * np.max(np.abs(wref))
        assert np.max(np.abs(A @ Z - Z * w)) < 1e-12
        assert np.max(np.abs(Z.T @ Z - np.eye(n))) < 1e-12


def test_restart_fill_and_breakdown(run):
    seen = set()
    for t, (k0, j0, al, be, Tm, broken) in enumerate(_restart_cases()):
        ma = M - k0
        jb, T = _fill_ref(Tm, k0, j0, al, be)
        assert (jb >= 0) == broken and (not broken or jb == j0 + 3)
        rc, r = run.results[run.ids["fill", t]]
        assert rc == jb
        np.testing.assert_array_equal(r.reshape(ma, ma, order="F"), T)
        seen.add((k0, j0 > k0, broken))
    assert len(seen) == 8


def test_restart_count_nkeep_arrowhead(run, tmp_path):
    rng = np.random.default_rng(3)
    drv = Driver()
    want = []
    tol = 1e-12
    for k0, nev in ((0, NEV), (6, 1), (0, 3)):
        ma = M - k0
        theta = np.sort(rng.normal(size=ma))
        theta[1] = 1e-13                     # under the eps^(2/3) floor
        Z = np.linalg.qr(rng.normal(size=(ma, ma)))[0]
        beta = 0.7
        # residuals |beta Z[ma-1, i]| on both sides of tol * max(eps23, |theta_i|)
        bound = tol * np.maximum(EPS23, np.abs(theta))
        factor = np.where(np.arange(ma) % 2 == 0, 2.0, 0.5)   # (index 1 passes only thanks to the floor)
        Z[ma - 1, :] = factor * bound / beta
        resid = np.abs(beta * Z[ma - 1, :nev])
        conv = int(np.sum(resid <= tol * np.maximum(EPS23, np.abs(theta[:nev]))))
        assert nev == 1 or 0 < conv < nev
        assert abs(beta * Z[ma - 1, 1]) > tol * abs(theta[1])
        drv.add("nconv", ma, nev, [beta], [tol], theta, Z)
        want.append((conv, None))
        nkeep = _nkeep_ref(ma, nev)
        drv.add("nkeep", ma, nev)
        want.append((nkeep, None))
        T = np.zeros((ma, ma))
        T[np.arange(nkeep), np.arange(nkeep)] = theta[:nkeep]
        T[nkeep, :nkeep] = T[:nkeep, nkeep] = beta * Z[ma - 1, :nkeep]
        drv.add("arrow", ma, nkeep, [beta], theta, Z, rng.normal(size=(ma, ma)))
        want.append((0, T))
    for ma, nev, nk in ((23, 6, 14), (17, 1, 9), (8, 6, 6), (7, 6, 6), (20, 6, 13)):
        assert _nkeep_ref(ma, nev) == nk
        drv.add("nkeep", ma, nev)
        want.append((nk, None))
    drv.run(run.exe, tmp_path / "restart.txt")
    for (rc, r), (wrc, wT) in zip(drv.results, want):
        assert rc == wrc
        if wT is not None:
            np.testing.assert_array_equal(r.reshape(wT.shape, order="F"), wT)


def test_screen_decision(run):
    labels = []
    for t, (label, _, _, _, expected) in enumerate(_screen_cases()):
        rc, _ = run.results[run.ids["screen", t]]
        assert rc == expected, (label, rc, expected)
        labels.append(label)
    assert labels == ["below", "none-converged", "undecided", "adversarial", "none-invariant"]


def test_screen_setup(run, tmp_path):
    """mp, verify, hint, cut, tprobe, maxsteps from their formulas."""
    from edgpu._lib import OPTIONS

    drv = Driver()
    want = []
    for m, nev, dim, opts, conv, ev, tol in [
            (23, 6, 495, 0, 6, -9.36, 1e-12), (23, 6, 495, 0, 5, -9.36, 1e-12),
            (23, 6, 8, 0, 6, 0.25, 1e-12), (8, 6, 8, 0, 6, 0.25, 1e-12), (23, 6, 32670, OPTIONS["eigh_no_verify"], 6, 3.0, 1e-3),
            (23, 6, 32670, OPTIONS["eigh_nohint"], 6, 3.0, 1e-12), (7, 6, 100, 0, 6, -1.0, 1e-12), (64, 60, 5000, 0, 60, -1.0, 1e-12)]:
        mp = min(m, 20, 64 - nev, dim - nev)
        verify = not (opts & OPTIONS["eigh_no_verify"]) and dim > nev + 2 and mp >= 3 and conv == nev
        hint = verify and nev + 1 < m and not (opts & OPTIONS["eigh_nohint"])
        cut = ev - 1e-11 * max(1.0, abs(ev))
        drv.add("setup", m, nev, dim, opts, conv, [ev], [tol])
        want.append((mp, [float(verify), float(hint), cut, max(tol, 1e-5), float(min(dim - nev, 400))]))
    drv.run(run.exe, tmp_path / "setup.txt")
    for (rc, r), (mp, rest) in zip(drv.results, want):
        assert rc == mp
        np.testing.assert_array_equal(r, rest)


def test_driver_clean_under_sanitizers(run):
    """The same driver and cases under AddressSanitizer + UBSan (host code
    with its own main): no report, same output."""
    exe = _build(run.dir, ("-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    out = subprocess.run([exe, str(run.dir / "cases.txt")], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stderr[-2000:]
    assert out.stdout == run.raw
