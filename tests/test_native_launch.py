"""_native.launch / _native.call: the one place where a call into liboctahip.so gets its context, its stream, its pointer
arguments and its error name."""
import ctypes
import types

import pytest


class _Stub:
    """Stands in for the loaded library: every symbol it knows records its arguments and returns `rc`."""

    def __init__(self, rc=0, names=("octa_x",)):
        self.calls = []
        for n in names:
            setattr(self, n, lambda *a, _n=n: (self.calls.append((_n, a)), rc)[1])

    def octa_last_error(self):
        return b"stub message"


@pytest.fixture
def stub(hip_lib_built, monkeypatch):
    from octa_autosegmentation_amd import _native

    def make(rc=0):
        s = _Stub(rc)
        monkeypatch.setattr(_native, "_lib", s)
        monkeypatch.setattr(_native, "ctx", lambda index=None: ("ctx", index))
        monkeypatch.setattr(_native, "current_stream_ptr", lambda: "stream")
        return s
    return make


def test_launch_and_call_marshal_their_arguments(stub):
    import torch
    from octa_autosegmentation_amd import _native
    s = stub()
    t = torch.zeros(3)
    n = ctypes.c_int(0)
    ref = ctypes.byref(n)
    dev = types.SimpleNamespace(index=5)
    assert _native.launch("octa_x", dev, t, None, 7, 0.5, ref) is None
    (name, a), = s.calls
    assert name == "octa_x"
    assert a[0] == ("ctx", 5) and a[-1] == "stream"              # the device's context first, the current stream last
    assert a[1] == t.data_ptr() and type(a[1]) is int and a[2] is None
    assert a[3] == 7 and type(a[3]) is int and a[4] == 0.5 and type(a[4]) is float and a[5] is ref
    assert len(a) == 7

    s.calls.clear()
    _native.launch("octa_x", dev, t, ctx="mine", stream="side")
    assert s.calls == [("octa_x", ("mine", t.data_ptr(), "side"))]

    s.calls.clear()
    assert _native.call("octa_x", t, None, 7, 0.5, ref, b"path") is None
    assert s.calls == [("octa_x", (t.data_ptr(), None, 7, 0.5, ref, b"path"))]      # neither context nor stream


def test_failure_names_the_symbol_or_the_given_label(stub):
    from octa_autosegmentation_amd import _native
    stub(rc=7)
    dev = types.SimpleNamespace(index=0)
    with pytest.raises(_native.OctaHipError) as e:
        _native.launch("octa_x", dev, 1)
    assert "octa_x failed" in str(e.value) and "rc=7" in str(e.value) and "stub message" in str(e.value)
    with pytest.raises(_native.OctaHipError) as e:
        _native.launch("octa_x", dev, 1, what="octa_x (data gradient)")
    assert "octa_x (data gradient) failed" in str(e.value) and "rc=7" in str(e.value)
    with pytest.raises(_native.OctaHipError) as e:
        _native.call("octa_x", 1, what="the label")
    assert "the label failed" in str(e.value) and "rc=7" in str(e.value)


def test_call_reports_the_librarys_own_message(hip_lib_built):
    """No GPU: a correctly sized, empty struct gets as far as the NULL-context check (tests/test_cabi.py pins the message)."""
    from octa_autosegmentation_amd import _native
    args = _native.Conv3x3Args(struct_size=ctypes.sizeof(_native.Conv3x3Args))
    with pytest.raises(_native.OctaHipError) as e:
        _native.call("octa_conv3x3_nhwc_fwd", None, ctypes.byref(args), None)
    assert "octa_conv3x3_nhwc_fwd: null pointer" in str(e.value) and "rc=-2" in str(e.value)


def test_unknown_symbol_raises(hip_lib_built):
    from octa_autosegmentation_amd import _native
    with pytest.raises(AttributeError):
        _native.call("octa_no_such_entry_point", 1)
    with pytest.raises(AttributeError):
        _native.launch("octa_no_such_entry_point", types.SimpleNamespace(index=0), 1, ctx="c", stream="s")


@pytest.mark.gpu
def test_launch_on_a_side_stream(hip_lib_built):
    """The smallest shape with odd, unequal sides through a converted call site: absent pointers (mul / add), the tensor's own device
    context and the stream picked up from torch's current one."""
    import torch
    import torch.nn.functional as F
    from octa_autosegmentation_amd.data import gpu_augment
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randint(0, 256, (2, 5, 7), device="cuda", generator=g, dtype=torch.uint8)
    want = F.interpolate(x.float().unsqueeze(1), size=(9, 11), mode="bilinear", align_corners=False).squeeze(1)
    on_default = gpu_augment.resize_bilinear(x, (9, 11))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        on_side = gpu_augment.resize_bilinear(x, (9, 11))
    side.synchronize()
    assert torch.equal(on_side, on_default)
    assert (on_side - want).abs().max().item() <= 1e-3          # tests/test_augment_gpu.py's bound for this op on uint8 input (values up to 255)
