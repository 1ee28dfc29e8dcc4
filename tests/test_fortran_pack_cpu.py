"""ed_gpu_pack_params (fortran/ed_gpu_hxv.f90) against EDConfig.to_ctypes():
the Fortran program ed_gpu_replay reads a model in the reference's array
shapes, packs it and writes the struct's bytes; they must equal the bytes the
Python side hands the same library.  Host code only: runs without a GPU."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

from edgpu.params import Bath, EDConfig, EdParams
from fortran_model import boundary_cases, replay_exe, write_model

CASES = boundary_cases()


def _pack(cfg, tmp_path):
    model, out = tmp_path / "model.bin", tmp_path / "params.bin"
    write_model(cfg, model)
    r = subprocess.run([replay_exe(), "pack", str(model), str(out)], capture_output=True, text=True, timeout=60)
    return r, out


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_pack_equals_to_ctypes(name, tmp_path):
    cfg = dict((c[0], c[1]) for c in CASES)[name]()
    r, out = _pack(cfg, tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    size = int(re.search(r"SIZE=(\d+)", r.stdout).group(1))
    assert size == ctypes.sizeof(EdParams)
    got = out.read_bytes()
    want = bytes(cfg.to_ctypes())
    assert len(got) == len(want) == size
    if got != want:        # name the first differing field before failing
        for fname, _ in EdParams._fields_:
            f = getattr(EdParams, fname)
            a, b = got[f.offset:f.offset + f.size], want[f.offset:f.offset + f.size]
            assert a == b, f"{name}: field {fname} differs"
    assert got == want


def test_case_set_is_not_vacuous():
    """The models distinguish every index order the packer reverses."""
    cfgs = [c[1]() for c in CASES]

    def any_(pred):
        return any(pred(c) for c in cfgs)

    assert any_(lambda c: c.Nspin == 2 and np.any(c.impHloc[0, 1] != c.impHloc[1, 0].T))
    assert any_(lambda c: c.Norb == 3)
    assert any_(lambda c: c.bath.u is not None and np.any(c.bath.u))
    assert any_(lambda c: c.bath.d is not None and np.any(c.bath.d))
    assert any_(lambda c: c.bath_type == "hybrid" and c.bath.e.shape[1] == 1 < c.Norb)
    assert any_(lambda c: c.bath_type == "replica" and np.any(np.imag(c.bath.h))
                and np.any(c.bath.h != np.transpose(c.bath.h, (1, 0, 3, 2, 4))))
    assert any_(lambda c: c.Jz_basis)
    # and the remaining inputs of the struct each take a non-default value somewhere
    assert any_(lambda c: not c.hfmode) and any_(lambda c: c.jhflag)
    assert any_(lambda c: c.bath.vr is not None and np.any(np.imag(c.bath.vr)))
    assert {c.ed_mode for c in cfgs} == {"normal", "superc", "nonsu2"}
    assert {c.bath_type for c in cfgs} == {"normal", "hybrid", "replica"}


def test_invalid_model_is_refused_loudly(tmp_path):
    """Norb=4: pack stops with the library's message (ed_gpu_init's check)."""
    cfg = EDConfig(Norb=4, Nbath=2)
    cfg.impHloc = np.zeros((1, 1, 4, 4), dtype=np.complex128)
    cfg.bath = Bath(e=np.zeros((1, 4, 2)), v=np.full((1, 4, 2), 0.5))
    r, out = _pack(cfg, tmp_path)
    assert r.returncode != 0
    assert "ED_GPU ERROR" in r.stdout and "invalid ed_params" in r.stdout, r.stdout + r.stderr
    assert "SIZE=" not in r.stdout and not out.exists()
