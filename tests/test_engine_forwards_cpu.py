"""The host-memory forwards of ``TsmEngine`` -- ``forward_host``, ``forward_features`` on an ndarray, ``forward_tap`` -- as the
sequence of C calls they make: entry point, memkind, layout, clips per ``max_clips`` chunk, where each chunk's input and output
start, ``normalize``, and the shapes returned.  No GPU and no library: the engine is made without ``__init__`` and its ``_lib`` is a
fake that records.  (First written against the forwards as they stood before they were split into input builders and output
runners, where it passed as it stands: the split changed no call.)"""
import ctypes as C

import numpy as np
import pytest

from workoutdetector_amd import _lib
from workoutdetector_amd.engine import TsmEngine

T, H, W, CLASSES, FEAT, MAX_CLIPS = 2, 32, 32, 5, 8, 3
CLIP_BYTES = T * 3 * H * W * 4
TAP_DIMS = (4, 2, 2, 8)


class RecordingLib:
    """What the forwards call of libtsm_hip.so; every call succeeds and is kept as (name, arguments behind the handle)."""

    def __init__(self):
        self.calls = []

    def tsm_forward(self, h, *args):
        self.calls.append(('tsm_forward',) + args)
        return 0

    def tsm_forward_features(self, h, *args):
        self.calls.append(('tsm_forward_features',) + args)
        return 0

    def tsm_forward_tap(self, h, x, memkind, layout, n, stage, buf, cap, shape, stream):
        self.calls.append(('tsm_forward_tap', x, memkind, layout, n, stage, buf, cap, stream))
        shape[:] = TAP_DIMS
        C.memset(buf, 0, 4 * int(np.prod(TAP_DIMS)))
        return 0


def make_engine(consensus_type='avg'):
    eng = TsmEngine.__new__(TsmEngine)
    eng._lib, eng._h, eng._finalized = RecordingLib(), C.c_void_p(1), True
    eng.num_class, eng.num_segments, eng.height, eng.width, eng.max_clips, eng.device = CLASSES, T, H, W, MAX_CLIPS, 0
    eng.planes, eng.feature_dim, eng.consensus_type, eng.temporal_pool = 3, FEAT, consensus_type, False
    eng.convnext_depths = eng.tdn_depths = None
    return eng


def clips_of(b):
    return np.zeros((b, T, 3, H, W), dtype=np.float32)


def chunks_of(b):
    return [(s, min(MAX_CLIPS, b - s)) for s in range(0, b, MAX_CLIPS)]


@pytest.mark.parametrize('b', [1, MAX_CLIPS, MAX_CLIPS + 1])
@pytest.mark.parametrize('consensus_type', ['avg', 'identity'])
def test_forward_host_calls_tsm_forward_once_per_chunk(b, consensus_type):
    eng, x = make_engine(consensus_type), clips_of(b)
    out = eng.forward_host(x)
    row = (T if consensus_type == 'identity' else 1) * CLASSES
    assert out.dtype == np.float32 and out.shape == ((b, T, CLASSES) if consensus_type == 'identity' else (b, CLASSES))
    assert eng._lib.calls == [('tsm_forward', x.ctypes.data + s * CLIP_BYTES, _lib.MEM_HOST, _lib.LAYOUT_NTCHW, n,
                               out.ctypes.data + s * row * 4, None) for s, n in chunks_of(b)]


def test_forward_host_passes_the_layout_on():
    eng = make_engine()
    x = np.zeros((2, T, H, W, 3), dtype=np.float32)
    out = eng.forward_host(x, layout=_lib.LAYOUT_NTHWC)
    assert out.shape == (2, CLASSES)
    assert eng._lib.calls == [('tsm_forward', x.ctypes.data, _lib.MEM_HOST, _lib.LAYOUT_NTHWC, 2, out.ctypes.data, None)]


@pytest.mark.parametrize('b', [1, MAX_CLIPS, MAX_CLIPS + 1])
@pytest.mark.parametrize('normalize', [False, True])
def test_forward_features_on_an_ndarray_calls_tsm_forward_features_once_per_chunk(b, normalize):
    eng, x = make_engine(), clips_of(b)
    out = eng.forward_features(x, normalize=normalize)
    assert out.dtype == np.float32 and out.shape == (b * T, FEAT)
    assert eng._lib.calls == [('tsm_forward_features', x.ctypes.data + s * CLIP_BYTES, _lib.MEM_HOST, _lib.LAYOUT_NTCHW, n,
                               out.ctypes.data + s * T * FEAT * 4, int(normalize), None) for s, n in chunks_of(b)]


@pytest.mark.parametrize('b', [1, MAX_CLIPS, MAX_CLIPS + 1])
def test_forward_tap_makes_one_call_for_all_clips(b):
    """Never chunked: the library itself refuses more than ``max_clips`` clips."""
    eng, x = make_engine(), clips_of(b)
    out = eng.forward_tap(x, 'layer1')
    assert out.dtype == np.float32 and out.shape == TAP_DIMS and not out.any()
    (name, addr, memkind, layout, n, stage, _buf, cap, stream), = eng._lib.calls
    assert (name, addr, memkind, layout, n, stage, stream) == ('tsm_forward_tap', x.ctypes.data, _lib.MEM_HOST, _lib.LAYOUT_NTCHW, b, b'layer1', None)
    assert cap == b * T * max(16 * 16 * 64, 8 * 8 * 256, H * W * 8)      # the stem conv's output, layer1's, eight floats a pixel


def test_refusals_make_no_call():
    eng = make_engine()
    with pytest.raises(ValueError, match='out= goes with a CUDA tensor'):
        eng.forward_features(clips_of(1), out=np.empty((T, FEAT), dtype=np.float32))
    with pytest.raises(ValueError, match='clips hold 7 float32 values'):
        eng.forward_host(np.zeros((1, 7), dtype=np.float32))
    with pytest.raises(ValueError, match='unknown layout 99'):
        eng.forward_features(clips_of(1), layout=99)
    eng._finalized = False
    for call in (lambda: eng.forward_host(clips_of(1)), lambda: eng.forward_features(clips_of(1), out=1), lambda: eng.forward_tap(clips_of(1), 'conv1')):
        with pytest.raises(_lib.TsmError, match='load_state_dict'):
            call()
    assert eng._lib.calls == []
