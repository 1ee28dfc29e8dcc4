"""Dense truth of the pair and inter-orbital susceptibility tests (test
infrastructure only): chi_truth.Truth extended, not edited.

For a (non-Hermitian) operator O, chi_O(tau) = <O(tau) O^+(0)>, kept states n
of weight w_n, m over the whole spectrum of the block that the seed reaches,
D = E_m - E_n, f = -expm1(-beta D), s(D) = f / D with s(0) = beta:

  seed O^+|n>, p = w_n |<m|O^+|n>|^2:
      tau_i += p exp(-tau_i D)           iv_0 += p s(D)
      iv_i  += -p f / (i v_i - D)        w_i  += -p f / (wr_i + i eps - D)
  seed O|n>,   p = w_n |<m|O|n>|^2:
      tau_i += p exp(-(beta - tau_i) D)  iv_0 += p s(D)
      iv_i  +=  p f / (i v_i + D)        w_i  +=  p f / (wr_i + i eps + D)

  pair[a]:   O = Delta_a = c_{a,up} c_{a,dw}; O^+|n> lives in (nup+1, ndw+1)
             (N+2 in nonsu2), O|n> in (nup-1, ndw-1) (N-2).
  exc[a,b]:  O = sum_sigma c^+_{a,sigma} c_{b,sigma}, a != b, both spins in one
             amplitude; both seeds stay in n's own block.

The amplitudes <m|op|n> are formed by the forward form
(chi_pair_host.forward_image: c / c^+ applied to the source rows one after the
other with their Jordan-Wigner signs) between the dense eigenvectors of the
two blocks: no Lanczos, no seed kernel, no gather form.

As chi_truth does, every compared array must not be swamped by a static pole:
the part from poles with |D| > 1e-6 is asserted to be >= 1e-3 of the array's
maximum (`PairTruth.shares`).

EPS: the broadening of the real-axis checks per model, the smallest of 0.01,
0.1, 0.2, 0.3, 0.5 at which the CPU replay holds 1e-5 (the table is in
test_chi_pair_cpu's docstring).
"""
from functools import lru_cache

import numpy as np

import chi_truth as ct
from chi_pair_host import forward_image

EPS = {"C1": 0.01, "C2": 0.01, "CN": 0.01}


def options(name, **kw):
    from edgpu.chi import ChiOptions

    return ChiOptions(Lmats=ct.LMATS, Ltau=ct.LTAU, Lreal=ct.LREAL, beta=ct.BETA, eps=EPS[name], **kw)


class PairTruth(ct.Truth):
    def __init__(self, name):
        self.__dict__.update(ct.truth(name).__dict__)     # the dense blocks, computed once
        self.by_q = {(s.q1, s.q2): s for s in self.secs}

    def _pair_block(self, sec, d):
        """isector of the block two particles away (d = +-1: one up and one down more / fewer), or None."""
        q = (sec.q1 + 2 * d, 0) if self.cfg.ed_mode == "nonsu2" else (sec.q1 + d, sec.q2 + d)
        t = self.by_q.get(q)
        return None if t is None else t.isector

    def _sum_ext(self, rows, copt):
        """rows: (weight, energy, isector, vector in the sector's row order).
        Returns {"pair": (iv, tau, w) with leading (Norb,), "exc": (Norb, Norb)}."""
        from edgpu.chi import bosonic_matsubara, tau_grid
        from edgpu.gf import realaxis

        No, Ns, beta = self.cfg.Norb, self.cfg.Ns, copt.beta
        vm, tg = bosonic_matsubara(beta, copt.Lmats), tau_grid(beta, copt.ltau)
        zr = realaxis(copt.wini, copt.wfin, copt.Lreal) + 1j * copt.eps
        shapes = {"pair": (No,), "exc": (No, No)}
        mk = lambda: {k: [np.zeros(s + (len(vm),), complex), np.zeros(s + (len(tg),)), np.zeros(s + (len(zr),), complex)]   # noqa: E731
                      for k, s in shapes.items()}
        full, dyn = mk(), mk()
        self.min_abs_d_pair, self.min_amp2 = np.inf, np.inf

        def kernels(D, sign):
            f = -np.expm1(-beta * D)
            with np.errstate(divide="ignore", invalid="ignore"):
                s = np.where(D == 0.0, beta, f / np.where(D == 0.0, 1.0, D))
            iv = np.empty((len(vm), len(D)), complex)
            iv[0] = s
            if sign > 0:
                iv[1:] = -f[None] / (1j * vm[1:, None] - D[None])
                tau = np.exp(-tg[:, None] * D[None])
                w = -f[None] / (zr[:, None] - D[None])
            else:
                iv[1:] = f[None] / (1j * vm[1:, None] + D[None])
                tau = np.exp(-(beta - tg[:, None]) * D[None])
                w = f[None] / (zr[:, None] + D[None])
            return iv, tau, w

        def add(key, at, wt, e, tsec, seed, sign):
            D = self.w[tsec] - e
            a2 = np.abs(self.v[tsec].conj().T @ seed) ** 2          # |<m|op|n>|^2
            K = kernels(D, sign)
            far = np.abs(D) > ct.DYNAMIC_D
            for g in range(3):
                full[key][g][at] += wt * (K[g] @ a2)
                dyn[key][g][at] += wt * (K[g][:, far] @ a2[far])
            return D, float(np.vdot(seed, seed).real)

        for wt, e, isec, vec in rows:
            sec = self.secs[isec - 1]
            vec = np.asarray(vec)
            for a in range(No):
                # Delta_a|n>: c on (a, dw), then c on (a, up); Delta_a^+|n>: c^+ on (a, up), then c^+ on (a, dw)
                for sign, image in ((-1, (a + Ns, 0, a, 0)), (+1, (a, 1, a + Ns, 1))):
                    tsec = self._pair_block(sec, sign)
                    if tsec is None:
                        continue
                    D, n2 = add("pair", (a,), wt, e, tsec, forward_image(self.maps[isec], self.maps[tsec], image, vec),
                                sign)
                    self.min_abs_d_pair = min(self.min_abs_d_pair, float(np.min(np.abs(D))))
                    self.min_amp2 = min(self.min_amp2, n2)
            for a in range(No):
                for b in range(No):
                    if a == b:
                        continue
                    m = self.maps[isec]
                    # O_ab^+|n> = sum_sigma c^+_b c_a|n> (c first), O_ab|n> = sum_sigma c^+_a c_b|n>
                    up = forward_image(m, m, (a, 0, b, 1), vec) + forward_image(m, m, (a + Ns, 0, b + Ns, 1), vec)
                    dn = forward_image(m, m, (b, 0, a, 1), vec) + forward_image(m, m, (b + Ns, 0, a + Ns, 1), vec)
                    _, n2 = add("exc", (a, b), wt, e, isec, up, +1)
                    add("exc", (a, b), wt, e, isec, dn, -1)
                    self.min_amp2 = min(self.min_amp2, n2)
        self.shares = {}
        for key, shape in shapes.items():
            for at in np.ndindex(*shape):
                if key == "exc" and at[0] == at[1]:
                    continue
                for g, grid in enumerate(("iv", "tau", "w")):
                    share = np.max(np.abs(dyn[key][g][at])) / np.max(np.abs(full[key][g][at]))
                    self.shares[(key, at, grid)] = share
                    assert share >= ct.DYNAMIC_SHARE, (self.name, key, at, grid, share)
        return {k: tuple(v) for k, v in full.items()}

    def pair_exc_of_list(self, states, copt, vector_of=None):
        """T = 0: the states of the list under test, w_n = 1/size."""
        from edgpu.diag import to_host

        assert not states.finite_t
        get = vector_of or (lambda k: np.asarray(to_host(states.vectors[k])))
        rows = [(1.0 / states.size, states.energies[k], states.sectors[k], get(k)) for k in range(states.size)]
        return self._sum_ext(rows, copt)

    def pair_exc_thermal(self, copt, cutoff=ct.CUTOFF):
        kept = self.thermal_states(copt.beta, cutoff)
        b = np.exp(-copt.beta * (np.array([t[0] for t in kept]) - self.e0))
        rows = [(bk / b.sum(), e, i, self.v[i][:, k]) for (e, i, k), bk in zip(kept, b)]
        return self._sum_ext(rows, copt)


@lru_cache(maxsize=None)
def truth(name) -> PairTruth:
    return PairTruth(name)


def distances(T, got, norb):
    """(d_iv, d_tau, d_w): over every compared component (every pair row, every
    off-diagonal exc entry), max |got - truth| over that array's own maximum."""
    d = [0.0, 0.0, 0.0]
    pairs = [(T["pair"], (got.pair_iv, got.pair_tau, got.pair_w), [(a,) for a in range(norb)]),
             (T["exc"], (got.exc_iv, got.exc_tau, got.exc_w), [(a, b) for a in range(norb) for b in range(norb) if a != b])]
    for tr, arrs, comps in pairs:
        for g in range(3):
            if arrs[g] is None:
                continue
            for at in comps:
                d[g] = max(d[g], np.max(np.abs(arrs[g][at] - tr[g][at])) / np.max(np.abs(tr[g][at])))
    return tuple(d)
