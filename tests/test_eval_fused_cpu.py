"""rx_eval_steps (ABI v25) without a GPU: the symbol, the version, the struct
layout and the argument checks that run before any HIP call."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from rx import _lib
    return _lib.load()


def test_symbol_and_version(L):
    from rx import _lib
    assert "rx_eval_steps" in _lib.EXPORTS
    assert hasattr(L, "rx_eval_steps")
    assert _lib.ABI_VERSION == 25 == L.rx_abi_version()
    src = open(os.path.join(ROOT, "include", "rx.h")).read()
    assert re.search(r"#define\s+RX_ABI_VERSION\s+25\b", src)
    assert re.search(r"#define\s+RX_EVAL_W\s+10\b", src) and _lib.RX_EVAL_W == 10


def test_struct_matches_the_header_layout():
    """rx_eval_io on LP64: two int32 (8 bytes) and nine pointers = 80 bytes, fields in the header's order."""
    from rx import _lib
    assert ctypes.sizeof(_lib.RxEvalIO) == 80
    src = open(os.path.join(ROOT, "include", "rx.h")).read()
    body = re.search(r"typedef struct rx_eval_io \{(.*?)\} rx_eval_io;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(\w+)\s*;", body)
    assert names == [n for n, _ in _lib.RxEvalIO._fields_]
    assert _lib.RxEvalIO.params.offset == 8 and _lib.RxEvalIO.n_active.offset == 72


def test_null_arguments_are_refused(L):
    from rx import _lib
    io, ev = _lib.RxIO(), _lib.RxEvalIO()
    # a stand-in for a handle: the checks below return before the handle is read
    h = ctypes.create_string_buffer(1 << 16)
    for args in ((None, ctypes.byref(io), ctypes.byref(ev)), (h, None, ctypes.byref(ev)),
                 (h, ctypes.byref(io), None)):
        assert L.rx_eval_steps(args[0], args[1], args[2], 1, None) == _lib.RX_EINVAL
        assert b"null" in L.rx_last_error()


def test_n_steps_and_obs_dim_are_refused_by_name(L):
    from rx import _lib
    io, ev = _lib.RxIO(), _lib.RxEvalIO()
    h = ctypes.create_string_buffer(1 << 16)
    for n in (0, -3):
        assert L.rx_eval_steps(h, ctypes.byref(io), ctypes.byref(ev), n, None) == _lib.RX_EINVAL
        assert b"n_steps" in L.rx_last_error()
    # every buffer present (never dereferenced on this path), policy mode, a width no policy kernel has
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    for k in ("obs", "reward64", "info", "done_f32"):
        setattr(io, k, p)
    for k, _ in _lib.RxEvalIO._fields_[2:]:
        setattr(ev, k, p)
    ev.obs_dim, ev.precision = 7, _lib.RX_PREC_FP32
    assert L.rx_eval_steps(h, ctypes.byref(io), ctypes.byref(ev), 1, None) == _lib.RX_EINVAL
    assert b"obs_dim" in L.rx_last_error()
    ev.obs_dim, ev.precision = 15, 5
    assert L.rx_eval_steps(h, ctypes.byref(io), ctypes.byref(ev), 1, None) == _lib.RX_EINVAL
    assert b"precision" in L.rx_last_error()
    # null buffers are named
    ev.precision = _lib.RX_PREC_FP32
    for k in ("actions", "acc", "active", "n_active", "log_std", "eps", "logp_sink", "value_sink"):
        setattr(ev, k, None)
        assert L.rx_eval_steps(h, ctypes.byref(io), ctypes.byref(ev), 1, None) == _lib.RX_EINVAL, k
        assert k.encode() in L.rx_last_error(), (k, L.rx_last_error())
        setattr(ev, k, p)
    for k in ("obs", "reward64", "info", "done_f32"):
        setattr(io, k, None)
        assert L.rx_eval_steps(h, ctypes.byref(io), ctypes.byref(ev), 1, None) == _lib.RX_EINVAL, k
        assert k.encode() in L.rx_last_error(), (k, L.rx_last_error())
        setattr(io, k, p)


def test_backend_argument_is_validated():
    """The backend name is checked before any env is built (no device needed)."""
    from rx.evaluate import Evaluator, MultiEvaluator
    for cls in (Evaluator, MultiEvaluator):
        with pytest.raises(ValueError, match="backend"):
            cls(num_tracks=1, num_runs=1, backend="graph")
