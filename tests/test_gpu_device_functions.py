"""Device against oracle, function by function: every small __device__ function that tests/probe/device_probe.hip wraps is run
on about 2^20 chosen inputs (tests/probe_inputs.py) in one launch and compared with the oracle's copy, by bits, under the three
rules of tests/probe_sets.py; then with the float64 models under the bounds the oracle holds on the CPU."""
import ctypes as C
import os

import numpy as np
import pytest

import probe_sets as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_LIB = os.environ.get("RADISH_PROBE_LIB") or os.path.join(ROOT, "tests", "probe", "libradish_probe.so")
SENTINEL = 0x5EA15EA1
PAD = 64  # words after the last record that must stay untouched
SIZES = (1, 63, 64, 65, 255, 256, 257, (1 << 20) + 1)


@pytest.fixture(scope="module")
def probe(gpu_ctx):
    import torch  # first: the library must bind to the HIP runtime torch ships, as api.Context's does

    if not os.path.exists(PROBE_LIB):
        pytest.fail(f"{PROBE_LIB} missing: __graft_entry__.build() (radish_pt_amd._build.build_probe) makes it")
    lib = C.CDLL(PROBE_LIB)
    for s in S.SPECS:
        fn = getattr(lib, s.entry())
        fn.argtypes, fn.restype = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p], C.c_int
    return lib, torch.cuda.Stream()


def run(probe, spec, inp):
    """One launch of spec's entry over `inp` on a non-default stream -> uint32 [n, words_out]; checks the padding."""
    import torch

    lib, stream = probe
    n = len(inp)
    buf = spec.device_buffer(inp)
    d_in = torch.from_numpy(buf.view(np.int32).copy()).cuda()
    d_out = torch.full((n * spec.words_out + PAD,), np.uint32(SENTINEL).astype(np.int32).item(), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = getattr(lib, spec.entry())(d_in.data_ptr(), d_out.data_ptr(), n, stream.cuda_stream)
    assert rc == 0, f"{spec.entry()} returned {rc}"
    stream.synchronize()
    out = d_out.cpu().numpy().view(np.uint32)
    assert (out[n * spec.words_out:] == SENTINEL).all(), f"{spec.entry()} wrote past record {n}"
    return out[:n * spec.words_out].reshape(n, spec.words_out)


_device = {}


def device_outputs(probe, spec):
    if spec.name not in _device:
        _device[spec.name] = run(probe, spec, spec.inputs())
    return _device[spec.name]


@pytest.mark.parametrize("spec", S.SPECS, ids=[s.name for s in S.SPECS])
def test_device_equals_oracle_by_bits(probe, spec):
    spec.compare(device_outputs(probe, spec), spec.oracle_outputs(), spec.inputs())


@pytest.mark.parametrize("spec", S.SPECS, ids=[s.name for s in S.SPECS])
def test_launch_sizes_and_padding(probe, spec):
    """n around the wave and workgroup sizes and one past 2^20: every record computed, nothing written after the n-th."""
    base = spec.inputs()
    for n in SIZES:
        inp = base[:n] if n <= len(base) else np.resize(base, (n, base.shape[1]))
        out = run(probe, spec, inp)
        if n <= len(base):
            full = device_outputs(probe, spec)[:n]
            assert np.array_equal(out, full), f"{spec.name}: n = {n} differs from the same records of the full launch"
        else:
            spec.compare(out, spec.oracle(inp), inp)


def test_entries_refuse_null_and_empty(probe):
    import torch

    lib, stream = probe
    d = torch.zeros(64, dtype=torch.int32, device="cuda")
    for s in S.SPECS:
        fn = getattr(lib, s.entry())
        assert fn(None, d.data_ptr(), 1, stream.cuda_stream) == -1
        assert fn(d.data_ptr(), None, 1, stream.cuda_stream) == -1
        assert fn(d.data_ptr(), d.data_ptr(), 0, stream.cuda_stream) == -1
        assert fn(d.data_ptr(), d.data_ptr(), -5, stream.cuda_stream) == -1
    torch.cuda.synchronize()
    assert (d == 0).all()


def test_device_holds_the_float64_bounds(probe):
    """The bounds the oracle holds on the CPU (tests/test_probe_inputs_cpu.py), applied to the device's outputs."""
    def outputs(name):
        out = device_outputs(probe, S.SPEC_BY_NAME[name])
        if name == "box":
            return out[:, 0].view(np.int32), out[:, 4].view(np.float32)
        return out

    S.assert_float64(S.float64_checks(outputs))
