"""CPU-side checks of graphed inference (no GPU): the predict() switch, the forward-only ABI entries and their argument checks."""
import ctypes
import inspect


def test_predict_has_use_graph_off_by_default():
    from model.mpnnlstm import NextFramePredictorS2S
    sig = inspect.signature(NextFramePredictorS2S.predict)
    assert list(sig.parameters)[1:] == ['loader', 'climatology', 'mask', 'high_interest_region', 'graph_structure', 'use_graph']
    assert sig.parameters['use_graph'].default is False
    assert callable(NextFramePredictorS2S.make_graphed_rollout)


def test_inference_entries_are_exported():
    from helpers import header_decls
    from qtmpnn import _lib
    decls = header_decls()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('qt_lstm_infer', 'qt_gather_frame'):
        assert hasattr(lib, name) and name in _lib.exported_names() and decls[name].times == 1, name


def _buf():
    """A 16-byte aligned host address that is only ever validated, never dereferenced (the calls fail their checks first)."""
    global _BUF
    _BUF = (ctypes.c_float * 64)()
    return ctypes.addressof(_BUF) + (-ctypes.addressof(_BUF)) % 16


def test_inference_entries_refuse_null_arguments():
    from qtmpnn import _lib
    lib = _lib.load()
    x = _buf()
    calls = {
        # O is required: the forward-only launches have no gate matrix to read it from
        'qt_lstm_infer': (x, None, 0, None, 0, x, x, None, 10, None, 16, None, x, x, None),
        'qt_gather_frame': (None, 1, 1, x, 1, 64, 10, None, 0, x, 0, 64, None),
    }
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == -1, name
        assert name.encode() in lib.qt_last_error(), (name, lib.qt_last_error())


def test_inference_entries_refuse_bad_arguments():
    from qtmpnn import _lib
    lib = _lib.load()
    x = _buf()
    # a hidden size the launch is not built for
    assert lib.qt_lstm_infer(x, None, 0, None, 0, x, x, None, 10, None, 12, x, x, x, None) == -1
    assert b'qt_lstm_infer' in lib.qt_last_error()
    # gather: row stride shorter than a row, an output slot that runs into the next clip, empty sizes
    assert lib.qt_gather_frame(x, 1, 4, x, 1, 64, 10, None, 0, x, 0, 256, None) == -1
    assert lib.qt_gather_frame(x, 4, 4, x, 2, 64, 10, None, 0, x, 256, 256, None) == -1
    assert lib.qt_gather_frame(x, 1, 1, x, 0, 64, 10, None, 0, x, 0, 64, None) == -1
    assert b'qt_gather_frame' in lib.qt_last_error()


def test_training_entry_still_needs_the_gate_matrix():
    """qt_lstm_fwd keeps its checks: no gate matrix, no launch (the forward-only entry is a separate one)."""
    from qtmpnn import _lib
    lib = _lib.load()
    x = _buf()
    assert lib.qt_lstm_fwd(x, None, 0, None, 0, x, x, None, 10, None, 16, x, x, x, None, None) == -1
    assert b'qt_lstm_fwd' in lib.qt_last_error()
