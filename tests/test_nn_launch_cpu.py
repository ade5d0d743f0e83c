"""CPU-side checks of the host layer in front of libgd_nn.so: the table from entry to error channel against the sources,
a rejected call that surfaces its own unit's text, the shared tensor-to-pointer conversion, and what nn_ops.py no longer
writes out by hand."""
import contextlib
import ctypes as C
import glob
import os
import re

import pytest
import torch

from garmentdreamer_amd import _launch, nn_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "garmentdreamer_amd", "csrc")


def _units():
    """{file name: (getter it defines, [entries it defines])} of csrc/nn_*.hip"""
    out = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "nn_*.hip"))):
        text = open(path).read()
        getters = re.findall(r"^const char\s*\*\s*(gd_nn_\w*last_error)\(", text, flags=re.M)
        entries = re.findall(r"^(?:int|size_t) (gd_nn_\w+)\(", text, flags=re.M)
        if getters or entries:
            out[os.path.basename(path)] = (getters, entries)
    return out


def test_channel_table_matches_the_sources():
    units = _units()
    assert units
    for name, (getters, _) in units.items():
        assert len(getters) == 1, (name, getters)
    getters = {g[0] for g, _ in units.values()}
    entries = [n for n in nn_ops.SIGNATURES if not n.endswith("_last_error")]
    assert entries and getters == set(nn_ops.SIGNATURES) - set(entries)
    for entry in entries:
        homes = [name for name, (_, defined) in units.items() if entry in defined]
        assert len(homes) == 1, (entry, homes)
        assert units[homes[0]][1].count(entry) == 1, entry
        assert nn_ops.error_channel(entry) == units[homes[0]][0][0], entry
    with pytest.raises(KeyError):
        nn_ops.error_channel("gd_nn_no_such_entry")


# one entry per translation unit, with arguments it rejects before any device work, and a piece of the text it leaves.
# P stands for a pointer that is not null (a host buffer nobody reads: the shape is refused first).
P = object()
REJECTED = [
    ("gd_nn_groupnorm_silu_forward", (None, None, None, None, None, 1, 64, 64, 32, 1e-5, 1, None, None), "null pointer"),
    ("gd_nn_conv3x3_forward", (None, None, None, None, 0, None, None, 1, 8, 8, 64, 64), "null pointer"),
    ("gd_nn_conv3x3_forward", (None, P, P, None, 0, None, P, 1, 8, 8, 63, 64), "conv3x3: need Cin % 64 == 0"),
    ("gd_nn_linear_k320_forward", (None, P, P, None, P, 0, 320), "linear_k320: need 0 < M"),
    ("gd_nn_gemm_forward", (None, None, None, None, None, None, 64, 64, 64), "gd_nn_gemm_forward: null pointer"),
    ("gd_nn_geglu_forward", (None, None, None, 4, 8), "geglu: null pointer"),
    ("gd_nn_attention_d64_forward", (None,) + (None,) * 5 + (1, 64, 64, 1, 64, 64, 64, 64, 64, 64, 64, 64, 0.125, 64),
     "attention: null pointer"),
    ("gd_nn_vae_prologue_forward", (None, None, None, 1, 8, 8, 8, 8), "vae_prologue: null pointer"),
    ("gd_nn_fp8_quantize", (None, None, None, 8, 1.0), "fp8 quantize: need n % 8 == 0"),
    ("gd_nn_lora_rowdot", (None, None, None, None, 4, 8, 1.0, 0), "lora_rowdot: null pointer"),
    ("gd_nn_vae_decoder_stem", (None, None, 0, 1.0, None, None, None, None, None, 1, 8, 8, 64),
     "vae_decoder_stem: null pointer"),
]


@pytest.mark.parametrize("name,args,piece", REJECTED, ids=[f"{n}-{i}" for i, (n, _, _) in enumerate(REJECTED)])
def test_rejected_call_raises_with_its_own_units_text(name, args, piece):
    L = nn_ops.lib()
    host = C.create_string_buffer(64)
    real = [C.addressof(host) if a is P else a for a in args]
    # the GroupNorm file's buffer (the old default of _check) holds another text than any case expects
    assert L.gd_nn_groupnorm_silu_forward(None, *[C.addressof(host)] * 4, 1, 64, 7, 1, 1e-5, 1, None, C.addressof(host)) == -1
    assert b"need C % 8 == 0" in L.gd_nn_last_error()
    ret = getattr(L, name)(*real)
    assert ret < 0
    own = getattr(L, nn_ops.error_channel(name))().decode()
    assert piece in own
    with pytest.raises(RuntimeError) as e:
        nn_ops._check(ret, name)
    assert str(e.value) == f"{name} failed ({ret}): {own}"
    assert nn_ops._check(0, name) == 0 and nn_ops._check(3, name) == 3


def test_rejected_calls_cover_every_unit():
    assert {nn_ops.error_channel(n) for n, _, _ in REJECTED} == {g[0] for g, _ in _units().values()}


def test_check_falls_back_to_the_groupnorm_channel_and_takes_a_named_one():
    L = nn_ops.lib()
    assert L.gd_nn_groupnorm_silu_forward(None, None, None, None, None, 1, 64, 64, 32, 1e-5, 1, None, None) == -1
    with pytest.raises(RuntimeError, match=r"not an entry failed \(-1\): null pointer"):
        nn_ops._check(-1, "not an entry")
    assert L.gd_nn_geglu_forward(None, None, None, 4, 8) == -1
    with pytest.raises(RuntimeError, match=r"something failed \(-1\): geglu: null pointer"):
        nn_ops._check(-1, "something", "gd_nn_elementwise_last_error")


def test_call_passes_stream_first_and_tensors_as_pointers(monkeypatch):
    seen = {}

    @contextlib.contextmanager
    def guard(dev):
        seen["guard"] = dev
        yield

    class Stream:
        cuda_stream = 1234

    def current_stream(dev):
        seen["stream_of"] = dev
        return Stream()

    monkeypatch.setattr(torch.cuda, "device", guard)
    monkeypatch.setattr(torch.cuda, "current_stream", current_stream)
    t = torch.zeros(4)
    view = t[1:]
    f, table = C.c_float(0.5), (C.c_ubyte * 4)()

    def fn(*args):
        seen["args"] = args
        return 7

    assert _launch.call(fn, "the device", (t, None, 3, 2.5, view, f, table)) == 7
    assert seen["guard"] == "the device" and seen["stream_of"] == "the device"
    args = seen["args"]
    assert args[0] == 1234
    assert args[1] == t.data_ptr() and args[5] == view.data_ptr() == t.data_ptr() + 4
    assert args[2] is None and args[3] == 3 and type(args[3]) is int and args[4] == 2.5
    assert args[6] is f and args[7] is table and len(args) == 8


def test_nn_ops_source_keeps_launch_plumbing_in_one_place():
    text = open(os.path.join(ROOT, "garmentdreamer_amd", "nn_ops.py")).read()
    assert "_check8" not in text and "_lora_check" not in text

    def body(name):
        m = re.search(rf"^def {name}\(.*?(?=^\S)", text, flags=re.M | re.S)
        assert m, name
        return m.group(0)

    rest = text.replace(body("_gn_workspace"), "").replace(body("launch"), "")
    assert "cuda_stream" not in rest and "with torch.cuda.device" not in rest
    assert "failed (" not in rest.replace(body("_check"), "")


def test_importing_nn_ops_loads_no_library():
    import subprocess
    import sys
    code = ("from garmentdreamer_amd import nn_ops, _native, _launch\n"
            "assert nn_ops._lib is None and _native._lib is None\n")
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True)
