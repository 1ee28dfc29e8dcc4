"""Host restatements for the pair / inter-orbital susceptibility tests (test
infrastructure only).

forward_image          one image op2_lev2 op1_lev1 |x> in the FORWARD form: over
                       the source rows, c / c^+ applied one after the other
                       with their Jordan-Wigner signs (the vvinit loops of the
                       reference), scattered into the target sector's rows.
                       The kernel and csrc/ed_seed_pair.hpp run the gather form.
numpy_pair_seeds       the unnormalised seeds of ed_sector_seed_pair from it.
chi_poles_host_signed  chi_host.chi_poles_host under the name these tests
                       use: fractions carry the isign selector of
                       ed_chi_add_poles_signed.
replay_chi_pair        build_chi(spin=False, dens=False, pair, exc) with every
                       device piece replaced: numpy seeds, the oracle's plain
                       Lanczos, `tridiag_poles`, chi_poles_host_signed.
"""
import numpy as np

from chi_host import chi_poles_host
from edgpu.chi import assemble, bosonic_matsubara, n_components, pair_target, seed_pair_calls, tau_grid
from edgpu.gf import _peso_bz, realaxis, tridiag_poles
from edgpu.sectors import setup_pointers


def _below(state, lev):
    """Number of occupied levels below `lev`, per state."""
    n = np.zeros(len(state), dtype=np.int64)
    for b in range(lev):
        n += (state >> b) & 1
    return n


def _ladder(state, lev, op):
    """c (op 0) or c^+ (op 1) on `lev` of every state: (allowed, new state, sign)."""
    ok = ((state >> lev) & 1) != op                 # c needs the level occupied, c^+ empty
    sign = 1.0 - 2.0 * (_below(state, lev) & 1)
    return ok, state ^ (1 << lev), sign


def forward_image(map_src, map_dst, image, x):
    """op2 on lev2 after op1 on lev1 of the vector x over map_src, on map_dst's rows (both ascending)."""
    lev1, op1, lev2, op2 = image
    s = np.asarray(map_src).astype(np.int64)
    ok1, mid, sg1 = _ladder(s, lev1, op1)
    ok2, t, sg2 = _ladder(mid, lev2, op2)
    ok = ok1 & ok2
    md = np.asarray(map_dst).astype(np.int64)
    out = np.zeros(len(md), dtype=np.asarray(x).dtype)
    if np.any(ok):
        rows = np.searchsorted(md, t[ok])
        assert np.array_equal(md[rows], t[ok]), "an image left the target sector"
        out[rows] = (sg1[ok] * sg2[ok]) * np.asarray(x)[ok]
    return out


def numpy_pair_seeds(map_src, map_dst, images, terms, x):
    """Unnormalised seeds (nseed, dim_dst) of the vector's type: image p, or image p + image q."""
    img = [forward_image(map_src, map_dst, im, x) for im in images]
    return np.array([img[p] if q < 0 else img[p] + img[q] for p, q in terms])


chi_poles_host_signed = chi_poles_host      # the isign element is the sixth of a fraction


def replay_chi_pair(cfg, states, copt, pair=True, exc=True, record=None):
    """The pair and inter-orbital parts of build_chi on the host, in its queue order."""
    from oracle.oracle import Oracle, lanc_tridiag
    from oracle_gf_superc import host_state_vector

    orc = Oracle(cfg)
    calls = seed_pair_calls(cfg, pair, exc)
    secs = setup_pointers(cfg)
    zeta = states.zeta if states.finite_t else float(states.size)
    fracs = []
    for k, isec in enumerate(states.sectors):
        sec = secs[isec - 1]
        hmap = orc.build_sector(sec.q1, sec.q2)
        vec = host_state_vector(cfg, orc, states, k, sign=False).astype(np.complex128)
        for target, images, terms, queue in calls:
            tsec = sec if target == 0 else pair_target(cfg, sec, target)
            if tsec is None:
                continue
            tmap = orc.build_sector(tsec.q1, tsec.q2)
            csr = orc.build_csr(tmap)
            nlanc = min(len(tmap), copt.lanc_nGFiter)
            seeds = numpy_pair_seeds(hmap, tmap, images, terms, vec)
            for s, v in enumerate(seeds):
                norm2 = float(np.vdot(v, v).real)
                if norm2 == 0.0:
                    continue
                a, b, n = lanc_tridiag(csr, v / np.sqrt(norm2), nlanc, copt.threshold)
                E, z = tridiag_poles(a, b, nlanc, first_row=True)
                for name, comp, isign in queue[s]:
                    if record is not None:
                        record.append(dict(name=name, comp=comp, state=k, isector=isec, norm2=norm2, alfa=a, beta=b,
                                           nlanc=n, isign=isign))
                    fracs.append((comp, _peso_bz(states, k, 1.0, norm2, zeta), states.energies[k], E, z, isign))
    vm, tg = bosonic_matsubara(copt.beta, copt.Lmats), tau_grid(copt.beta, copt.ltau)
    wr = realaxis(copt.wini, copt.wfin, copt.Lreal)
    iv, tau, w, _ = chi_poles_host_signed(fracs, copt.beta, vm, tg, wr, copt.eps, n_components(cfg, pair, exc))
    return assemble(cfg, copt, iv, tau, w, spin=False, dens=False, pair=pair, exc=exc)
