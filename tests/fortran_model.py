"""The model file of fortran/ed_gpu_replay and the readers of its raw outputs.

write_model(cfg, path) writes an EDConfig as the Fortran program reads it: a
header of int32 values, the scalars, then every array as float64 in the
reference's Fortran shape and element order (ED_BATH/dmft_aux.f90:13-44), so
that ed_gpu_pack_params receives exactly what the reference would hand it.
The comparisons are in the tests (test_fortran_pack_cpu.py,
test_gpu_fortran_modes.py).
"""
import os
import re
import subprocess

import numpy as np

from edgpu.params import BATHS, MODES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPLAY = os.path.join(ROOT, "dmft-ed_amd", "fortran", "ed_gpu_replay")


def boundary_cases():
    """(name, EDConfig factory, sectors): every entry of cases.CASES, the
    complex-vr replica model and one adversarial (equal bath pairs) model."""
    import json

    import cases
    from golden.golden_configs import ADV_SECTOR, adv_config

    with open(os.path.join(ROOT, "tests", "golden", "adversarial_probe.json")) as f:
        ed = json.load(f)["cases"][0]["ed"]
    return list(cases.CASES) + [
        ("replica_cplx_vr", cases.replica_cplx_vr, [(3, 3), (2, 4)]),
        ("adversarial", lambda: adv_config(ed), [ADV_SECTOR]),
    ]


def replay_exe():
    if not os.path.exists(REPLAY):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "dmft-ed_amd"), "fortran"], check=True)
    return REPLAY


def run_replay(*args, timeout=300):
    """One child process.  A child that was killed by a signal or ran out of
    time may have left the GPU faulted: the whole session ends there, no
    later test starts anything on it."""
    import pytest

    cmd = [replay_exe(), *map(str, args)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        pytest.exit(f"{' '.join(cmd)}: no end within {timeout} s", returncode=1)
    if r.returncode < 0 or r.returncode in (134, 139):
        pytest.exit(f"{' '.join(cmd)}: died with {r.returncode}\n{r.stdout}{r.stderr}", returncode=1)
    return r


def _f(a, dtype):
    """Fortran element order of a numpy array indexed as the reference indexes it."""
    return np.asarray(a, dtype=dtype).ravel(order="F").tobytes()


def write_model(cfg, path):
    """No cfg.check(): an invalid model (Norb=4) is written as it is."""
    b = cfg.bath
    No, Ns, Nb = cfg.Norb, cfg.Nspin, cfg.Nbath
    ne = 0 if b.e is None else b.e.shape[1]
    assert (b.e is None) == (b.v is None) and (b.h is None) == (b.vr is None)
    hdr = [No, Ns, Nb, MODES[cfg.ed_mode], BATHS[cfg.bath_type], int(bool(cfg.hfmode)),
           int(bool(cfg.Jz_basis)), ne, int(b.u is not None), int(b.d is not None), int(b.h is not None)]
    himp = cfg.impHloc if cfg.impHloc is not None else np.zeros((Ns, Ns, No, No))
    assert np.shape(himp) == (Ns, Ns, No, No)
    with open(path, "wb") as f:
        f.write(np.array(hdr, dtype=np.int32).tobytes())
        f.write(np.array([*cfg.Uloc[:3], cfg.Ust, cfg.Jh, cfg.Jx, cfg.Jp, cfg.xmu], dtype=np.float64).tobytes())
        f.write(_f(himp, np.complex128))
        if ne:
            assert b.e.shape == (Ns, ne, Nb) and b.v.shape == (Ns, No, Nb)
            f.write(_f(b.e, np.float64))
            f.write(_f(b.v, np.float64))
        if b.u is not None:
            assert b.u.shape == (Ns, No, Nb)
            f.write(_f(b.u, np.float64))
        if b.d is not None:
            assert b.d.shape == (Ns, ne, Nb)
            f.write(_f(b.d, np.float64))
        if b.h is not None:
            assert b.h.shape == (Ns, Ns, No, No, Nb) and b.vr.shape == (Nb,)
            f.write(_f(b.h, np.complex128))
            f.write(_f(b.vr, np.complex128))


# ------------------------------------------------------------- raw outputs
def _bin(outdir, stem, q1, q2, dtype):
    return np.fromfile(os.path.join(outdir, f"{stem}_{q1}_{q2}.bin"), dtype=dtype)


def read_hv(outdir, q1, q2):
    return _bin(outdir, "hv", q1, q2, np.complex128)


def read_rows(outdir, nproc, q1, q2):
    return _bin(outdir, f"hvrows_{nproc}", q1, q2, np.complex128)


def read_csr(outdir, q1, q2):
    return (_bin(outdir, "csr_rowptr", q1, q2, np.int64), _bin(outdir, "csr_cols", q1, q2, np.int32),
            _bin(outdir, "csr_vals", q1, q2, np.complex128))


def read_tridiag(outdir, q1, q2, nsteps=40):
    ab = _bin(outdir, "tri", q1, q2, np.float64)
    assert ab.shape == (2 * nsteps,)
    return ab[:nsteps], ab[nsteps:]


def parse_lines(stdout, key):
    """{(q1, q2): {NAME: text}} of the program's `KEY=q1,q2 NAME=value ...`
    lines; the ROWS lines, several per sector, are keyed (q1, q2, RANKS)."""
    out = {}
    for line in stdout.splitlines():
        m = re.match(rf"\s*{key}=(-?\d+),(-?\d+)\s+(.*)", line)
        if not m:
            continue
        vals = dict(re.findall(r"(\w+)=\s*(\S+)", m.group(3)))
        k = (int(m.group(1)), int(m.group(2)))
        if key == "ROWS":
            k += (int(vals["RANKS"]),)
        assert k not in out, line
        out[k] = vals
    return out
