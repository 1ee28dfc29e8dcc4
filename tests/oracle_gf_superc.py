"""edgpu.gf.build_gf_superc job runner from the oracle pieces (test
infrastructure): one seed of lanc_build_gf_superc_c (ED_GF_SUPERC.f90:88-446)
built term by term with oracle_gf.seed (each term with its own operator type),
tridiagonalised by the oracle's plain Lanczos, poles by the oracle's tql2 and
the weight of add_to_lanczos_gf_superc (ED_GF_SUPERC.f90:757-803): norm2 / zeta
at T = 0, norm2 exp(-beta (E_n - E_gs)) / zeta at finite T, with no
beta dE < 200 cut.

A twin entry's vector is its partner's reordered on the host: row i of the
twin sector holds state s and takes the partner's value at flip_state(s), the
two Ns-bit halves exchanged (es_return_cvector, ED_EIGENSPACE.f90:414-445;
twin_sector_order / flip_state, ED_SETUP.f90:1123-1186), times
edgpu.gf.superc_twin_sign: the exchange of the spin halves alone maps
H(deltasc) to H(-deltasc), and the reordered vector is an eigenvector only
with that sign (test_superc_gf_cpu checks the residual both ways).
"""
import numpy as np

from edgpu.diag import to_host
from edgpu.gf import superc_twin_sign
from edgpu.sectors import setup_pointers
from oracle.oracle import Oracle, lanc_tridiag, tql2
from oracle_gf import seed


def host_state_vector(cfg, orc, states, k, sign=True):
    p = states.partner(k)
    if p is None:
        return np.asarray(to_host(states.vectors[k]))
    secs = setup_pointers(cfg)
    src, dst = secs[states.sectors[p] - 1], secs[states.sectors[k] - 1]
    Ns = cfg.Ns
    map_src, map_dst = orc.build_sector(src.q1, src.q2), orc.build_sector(dst.q1, dst.q2)
    low = np.uint32((1 << Ns) - 1)
    flipped = ((map_dst & low) << np.uint32(Ns)) | (map_dst >> np.uint32(Ns))
    rows = np.searchsorted(map_src, flipped)
    assert np.array_equal(map_src[rows], flipped)
    v = np.asarray(to_host(states.vectors[p]))[rows]
    return v * superc_twin_sign(Ns, map_dst) if sign else v


def peso_superc(states, k, norm2, zeta):
    if not states.finite_t:
        return norm2 / zeta
    return norm2 * np.exp(-states.beta * (states.energies[k] - states.emin)) / zeta


def oracle_job_runner_superc(cfg, states, gopt, job, wm, wr, G_m, G_r, zeta):
    comp, tag, k, (op, isign, ispin, terms, weight), sec, jsec = job
    orc = Oracle(cfg)
    hmap_i = orc.build_sector(sec.q1, sec.q2)
    vec = host_state_vector(cfg, orc, states, k).astype(np.complex128)
    v = None
    for level, coef, op_t in terms:
        hmap_j, w = seed(orc, hmap_i, jsec, op_t, level, vec)
        v = coef * w if v is None else v + coef * w
    norm2 = float(np.vdot(v, v).real)
    if norm2 == 0.0:
        return
    v = v / np.sqrt(norm2)
    nlanc = min(len(hmap_j), gopt.lanc_nGFiter)
    a, b, n = lanc_tridiag(orc.build_csr(hmap_j), v, nlanc, gopt.threshold)
    E, Z, ierr = tql2(a[:nlanc], np.concatenate([[0.0], b[1:nlanc]]))
    de = E - states.energies[k]
    peso = weight * peso_superc(states, k, norm2, zeta) * Z[0, :] ** 2
    G_m += (peso[None] / ((1j * wm)[:, None] - isign * de[None])).sum(1)
    G_r += (peso[None] / ((wr + 1j * gopt.eps)[:, None] - isign * de[None])).sum(1)
