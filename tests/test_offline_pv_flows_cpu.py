"""What each of the seven phase-vocoder flows of vocoderproject_amd.offline hands to its processor and gives back, and every ValueError it
raises: pv_shift, pv_glide, pv_shift_locked, pv_shift_formant (batch and stream), pv_stretch, pv_autotune, pv_autotune_stream.  The
processors are recording stand-ins; the recordings have unequal lengths, one of a single sample and one shorter than a frame.  The
expected arrays are worked out here from the flows' documented arithmetic, not taken from the module."""
import numpy as np
import pytest

from vocoderproject_amd import offline

LENS = (1, 300, 2500)
VOICES = [((np.arange(n) % 97 + 1) / 128.0 * (-1) ** s).astype(np.float32) for s, n in enumerate(LENS)]
S = len(VOICES)
NO_REC = "no recordings"
MONO = r"voice 1: expected a mono signal, got shape \(2, 5\)"
BAD_VOICES = [VOICES[0], np.zeros((2, 5), np.float32), VOICES[2]]
FORMANT_MSG = "formant: an interval within +-12 semitones expected"
LIFTER_MSG = "lifter: 4 to 64 samples expected"
LOCK_FORMANT_MSG = "--locked and --formant exclude each other: formant correction on top of peak locking is not built"
LOCK_2K_MSG = "--locked: 1024-point frames expected (the peak-locked kernels are not built for 2048)"
SHIFT_COUNT_MSG = "shift: one value per recording expected"
SHIFT_RANGE_MSG = "shift: intervals within +-12 semitones expected"
KEY_COUNT_MSG = "key: one value per recording expected"
KEY_RANGE_MSG = "key: 0..12 expected (12 = chromatic)"
FS_MSG = "pvtune: sample rates from 8000 to 51200 Hz are served"


def raises(msg, fn, *a, **kw):
    with pytest.raises(ValueError) as e:
        fn(*a, **kw)
    assert str(e.value) == msg, (str(e.value), msg)


def padded(T):
    x = np.zeros((S, T), np.float32)
    for s, v in enumerate(VOICES):
        x[s, :v.size] = v
    return x


def is_batch(x, T):
    assert isinstance(x, np.ndarray) and x.dtype == np.float32 and x.shape == (S, T) and x.flags.c_contiguous, (x.dtype, x.shape)
    assert np.array_equal(x, padded(T))                       # the recordings in front, zeros behind


def both_channels(outs, rows, lens=LENS, offset=0):
    assert len(outs) == S
    for s, o in enumerate(outs):
        assert o.dtype == np.float32 and o.shape == (2, lens[s]) and o.flags.c_contiguous, (s, o.dtype, o.shape)
        assert np.array_equal(o[0], rows[s][offset:offset + lens[s]]) and np.array_equal(o[1], o[0]), s


class _Blocks:
    """PhaseVocoderStream's interface as pv_shift uses it: a pure delay of `latency` samples."""
    latency = 768

    def __init__(self):
        self.set, self.blocks, self.hist = [], [], None

    def set_semitones(self, v, stream=-1):
        self.set.append((v, stream))

    def process(self, x):
        assert x.dtype == np.float32 and x.flags.c_contiguous
        self.blocks.append(x.copy())
        if self.hist is None:
            self.hist = np.zeros((x.shape[0], self.latency), np.float32)
        cat = np.concatenate([self.hist, x], axis=1)
        self.hist = cat[:, x.shape[1]:]
        return np.ascontiguousarray(cat[:, :x.shape[1]])


class _Stream:
    """PhaseVocoderStream's interface as the streamed flows use it: run() returns its input, aligned."""
    latency = 768

    def __init__(self):
        self.calls = []

    def run(self, x, *a, **kw):
        self.calls.append((x.copy(), a, kw))
        return x.copy()


class _OneShot:
    """The one-shot runners' interface: run() keeps its arguments and returns what `result` makes of them."""

    def __init__(self, result):
        self.calls, self.result = [], result

    def run(self, *a, **kw):
        self.calls.append((a, kw))
        return self.result(*a)


def test_pv_shift():
    N = 256
    T = 13 * N                                                # ceil((2500 + 768) / 256) blocks
    for shift, want in ((3.0, [3.0] * 3), ([3, -2.0, 12], [3.0, -2.0, 12.0]), ((0.5, 1.5, -12.0), [0.5, 1.5, -12.0])):
        p = _Blocks()
        outs = offline.pv_shift(VOICES, shift, N=N, processor=p)
        assert p.set == [(v, s) for s, v in enumerate(want)] and all(type(v) is float for v, _ in p.set)
        assert len(p.blocks) == 13 and all(b.shape == (S, N) for b in p.blocks)
        is_batch(np.ascontiguousarray(np.concatenate(p.blocks, axis=1)), T)
        both_channels(outs, VOICES)
    raises(NO_REC, offline.pv_shift, [], 1.0, processor=_Blocks())
    raises(SHIFT_COUNT_MSG, offline.pv_shift, VOICES, [1.0, 2.0], processor=_Blocks())
    raises(SHIFT_COUNT_MSG, offline.pv_shift, VOICES, (1.0, 2.0, 3.0, 4.0), processor=_Blocks())
    with pytest.raises(ValueError, match=MONO):
        offline.pv_shift(BAD_VOICES, 1.0, processor=_Blocks())


def glide(start, end, N, n_blocks):
    c = np.empty((n_blocks, S))
    for s, n in enumerate(LENS):
        nb = max(1, -(-n // N))
        for b in range(n_blocks):
            c[b, s] = start + (end - start) * min(b / max(nb - 1, 1), 1.0)
    return c


def test_pv_glide():
    for N, nblk in ((256, 13), (1024, 4)):                    # ceil((2500 + 768) / N)
        for extra, kw in ((dict(), {}), (dict(formant=2, lifter=16.0), dict(formant_semitones=2.0, lifter=16)), (dict(locked=True), dict(locked=True)),
                          (dict(formant=None, lifter=99, locked=False), {})):
            p = _Stream()
            outs = offline.pv_glide(VOICES, -12, 7.5, N=N, processor=p, **extra)
            (x, a, k), = p.calls
            is_batch(x, 2500)
            assert a == () and set(k) == {"blocks_per_call", "curve"} | set(kw) and k["blocks_per_call"] == 16 and type(k["blocks_per_call"]) is int
            assert k["curve"].dtype == np.float64 and k["curve"].shape == (nblk, S) and np.array_equal(k["curve"], glide(-12.0, 7.5, N, nblk))
            for name, v in kw.items():
                assert k[name] == v and type(k[name]) is type(v), name
            both_channels(outs, VOICES)
    p = _Stream()
    offline.pv_glide(VOICES, 0.0, 1.0, blocks_per_call=3, processor=p)
    assert p.calls[0][2]["blocks_per_call"] == 3
    raises(NO_REC, offline.pv_glide, [], 0.0, 1.0, processor=_Stream())
    for a, b in ((-12.5, 0.0), (0.0, 12.5), (float("nan"), 0.0)):
        raises("glide: intervals within +-12 semitones expected", offline.pv_glide, VOICES, a, b, processor=_Stream())
    raises(FORMANT_MSG, offline.pv_glide, VOICES, 0.0, 1.0, formant=12.5, processor=_Stream())
    raises(FORMANT_MSG, offline.pv_glide, VOICES, 0.0, 1.0, formant=-13, lifter=3, locked=True, processor=_Stream())   # (the first check wins)
    raises(LIFTER_MSG, offline.pv_glide, VOICES, 0.0, 1.0, formant=0.0, lifter=3, processor=_Stream())
    raises(LIFTER_MSG, offline.pv_glide, VOICES, 0.0, 1.0, formant=0.0, lifter=65, locked=True, processor=_Stream())
    raises(LOCK_FORMANT_MSG, offline.pv_glide, VOICES, 0.0, 1.0, formant=0.0, locked=True, processor=_Stream())
    with pytest.raises(ValueError, match=MONO):
        offline.pv_glide(BAD_VOICES, 0.0, 1.0, processor=_Stream())


def test_pv_shift_locked():
    for shift, want in ((7, [7.0] * 3), ([3.0, -2.0, 12.0], [3.0, -2.0, 12.0]), (np.array([1, 2, 3]), [1.0, 2.0, 3.0])):
        p = _Stream()
        outs = offline.pv_shift_locked(VOICES, shift, N=256, processor=p)
        (x, a, k), = p.calls
        is_batch(x, 2500)
        assert a == () and set(k) == {"blocks_per_call", "curve", "locked"} and k["blocks_per_call"] == 16 and k["locked"] is True
        assert k["curve"].dtype == np.float64 and k["curve"].shape == (1, S) and k["curve"].tolist() == [want]
        both_channels(outs, VOICES)
    raises(NO_REC, offline.pv_shift_locked, [], 0.0, processor=_Stream())
    raises(SHIFT_COUNT_MSG, offline.pv_shift_locked, VOICES, [0.0, 13.0], processor=_Stream())       # (the count before the range)
    for shift in (12.5, [0.0, -12.5, 0.0], float("nan")):
        raises(SHIFT_RANGE_MSG, offline.pv_shift_locked, VOICES, shift, processor=_Stream())
    with pytest.raises(ValueError, match=MONO):
        offline.pv_shift_locked(BAD_VOICES, 1.0, processor=_Stream())


def test_pv_shift_formant():
    for hop, T in ((256, 1024 + 10 * 256), (128, 1024 + 20 * 128)):                                  # batch: 1024 + ceil(2500 / hop) hop
        for shift, want in ((-5, [-5.0] * 3), ((1.0, 2.0, 3.0), [1.0, 2.0, 3.0])):
            p = _OneShot(lambda x, st, f, lf: x.copy())
            outs = offline.pv_shift_formant(VOICES, shift, formant=2, lifter=8.0, hop=hop, processor=p)
            ((x, st, f, lf), kw), = p.calls
            is_batch(x, T)
            assert kw == {} and st == want and all(type(v) is float for v in st) and (f, lf) == (2.0, 8) and type(f) is float and type(lf) is int
            both_channels(outs, VOICES)
    p = _OneShot(lambda x, st, f, lf: x.copy())
    offline.pv_shift_formant(VOICES, 0.0, processor=p)
    assert p.calls[0][0][2:] == (0.0, 32)
    p = _Stream()
    outs = offline.pv_shift_formant(VOICES, [3.0, -2.0, 12.0], formant=-1.0, lifter=64, N=256, stream=True, processor=p)
    (x, a, k), = p.calls
    is_batch(x, 2500)
    assert a == () and set(k) == {"blocks_per_call", "curve", "formant_semitones", "lifter"} and k["blocks_per_call"] == 16
    assert k["curve"].dtype == np.float64 and k["curve"].tolist() == [[3.0, -2.0, 12.0]] and (k["formant_semitones"], k["lifter"]) == (-1.0, 64)
    both_channels(outs, VOICES)
    raises(NO_REC, offline.pv_shift_formant, [], 0.0, processor=_Stream())
    raises(SHIFT_COUNT_MSG, offline.pv_shift_formant, VOICES, [0.0, 13.0], processor=_Stream())
    raises(SHIFT_RANGE_MSG, offline.pv_shift_formant, VOICES, -12.5, formant=13.0, processor=_Stream())
    raises(FORMANT_MSG, offline.pv_shift_formant, VOICES, 0.0, formant=13.0, lifter=3, processor=_Stream())
    raises(FORMANT_MSG, offline.pv_shift_formant, VOICES, 0.0, formant=float("nan"), processor=_Stream())
    for lifter in (3, 65):
        raises(LIFTER_MSG, offline.pv_shift_formant, VOICES, 0.0, lifter=lifter, processor=_Stream())
    for stream in (False, True):
        with pytest.raises(ValueError, match=MONO):
            offline.pv_shift_formant(BAD_VOICES, 1.0, stream=stream, processor=_Stream())


def test_pv_stretch():
    def ramp(x, pos, T, st):
        return (np.arange(x.shape[0] * T, dtype=np.float32) / 64.0).reshape(x.shape[0], T)
    for F, hop in ((1024, 256), (2048, 512), (1024, 64)):
        for stretch, per in ((1.5, [1.5] * 3), ([4.0, 0.25, 0.7], [4.0, 0.25, 0.7]), (np.array([1.0, 2.0, 0.5]), [1.0, 2.0, 0.5])):
            for locked in (False, True):
                if locked and F != 1024:
                    continue
                p = _OneShot(ramp)
                outs = offline.pv_stretch(VOICES, stretch, shift=3, F=F, hop=hop, processor=p, **({"locked": True} if locked else {}))
                lens = [int(np.ceil(n * a)) for n, a in zip(LENS, per)]
                T = F + -(-max(lens) // hop) * hop
                nF = (T - F) // hop + 1
                ((x, pos, T_got, st), kw), = p.calls
                is_batch(x, max(2500, F))
                assert kw == ({"locked": True} if locked else {}) and T_got == T and type(T_got) is int and st == 3.0 and type(st) is float
                want = np.array([[min(int(np.floor(f * hop / a)), max(n, F) - F) for f in range(nF)] for n, a in zip(LENS, per)])
                assert pos.dtype == np.int32 and pos.shape == (S, nF) and np.array_equal(pos, want)
                both_channels(outs, ramp(x, pos, T, st), lens=lens)
    p = _OneShot(ramp)
    offline.pv_stretch(VOICES, 1.0, processor=p)
    assert p.calls[0][0][3] == 0.0
    raises(NO_REC, offline.pv_stretch, [], 1.0, processor=_OneShot(ramp))
    raises("stretch: one value per recording expected", offline.pv_stretch, VOICES, [1.0, 5.0], processor=_OneShot(ramp))
    for stretch in (0.2, 4.5, [1.0, 1.0, 0.1], float("nan")):
        raises("stretch: factors within [0.25, 4] expected", offline.pv_stretch, VOICES, stretch, shift=13.0, processor=_OneShot(ramp))
    for shift in (12.5, -12.5, float("nan")):
        raises("shift: an interval within +-12 semitones expected", offline.pv_stretch, VOICES, 1.0, shift=shift, F=2048, locked=True, processor=_OneShot(ramp))
    raises(LOCK_2K_MSG, offline.pv_stretch, VOICES, 1.0, F=2048, hop=512, locked=True, processor=_OneShot(ramp))
    with pytest.raises(ValueError, match=MONO):
        offline.pv_stretch(BAD_VOICES, 1.0, processor=_OneShot(ramp))


def tune_result(shape_of):
    def result(x, fs, keys):
        shape = shape_of(x)
        return x.copy(), np.arange(shape[0] * shape[1], dtype=np.int32).reshape(shape), np.arange(shape[0] * shape[1], dtype=np.float64).reshape(shape) / 7.0
    return result


TUNE_EXTRAS = ((dict(), {}), (dict(formant=1, lifter=8.0), dict(formant=1.0, lifter=8)), (dict(locked=True), dict(locked=True)),
               (dict(formant=None, lifter=99, locked=False), {}))


def tune_common(fn, stub):
    for extra, kw in TUNE_EXTRAS:
        for key, keys in ((5, [5] * 3), ([0, 12, 7], [0, 12, 7]), (np.array([1, 2, 3]), [1, 2, 3])):
            yield extra, kw, key, keys
    raises(NO_REC, fn, [], 44100.0, processor=stub())
    raises(KEY_COUNT_MSG, fn, VOICES, 44100.0, key=[1, 13], processor=stub())
    for key in (-1, 13, [0, 1, 13]):
        raises(KEY_RANGE_MSG, fn, VOICES, 7999.0, key=key, processor=stub())
    for fs in (7999.0, 51201.0, float("nan")):
        raises(FS_MSG, fn, VOICES, fs, formant=13.0, processor=stub())
    raises(FORMANT_MSG, fn, VOICES, 44100.0, formant=-12.5, lifter=3, processor=stub())
    for lifter in (3, 65):
        raises(LIFTER_MSG, fn, VOICES, 44100.0, formant=0.0, lifter=lifter, locked=True, processor=stub())
    raises(LOCK_FORMANT_MSG, fn, VOICES, 44100.0, formant=0.0, locked=True, processor=stub())
    with pytest.raises(ValueError, match=MONO):
        fn(BAD_VOICES, 44100.0, processor=stub())


def test_pv_autotune():
    def stub(F=1024, hop=256):
        return _OneShot(tune_result(lambda x: (x.shape[0], (x.shape[1] - F) // hop + 1)))
    for fs, F, hop, T in ((44100, 1024, 256, 1024 + 10 * 256), (8000.0, 2048, 512, 2048 + 5 * 512), (51200.0, 1024, 128, 1024 + 20 * 128)):
        for extra, kw, key, keys in tune_common(offline.pv_autotune, stub):
            if F != 1024 and kw:
                continue
            p = stub(F, hop)
            outs, period, ratio = offline.pv_autotune(VOICES, fs, key=key, F=F, hop=hop, processor=p, with_track=True, **extra)
            ((x, fs_got, keys_got), kw_got), = p.calls
            is_batch(x, T)
            assert fs_got == float(fs) and type(fs_got) is float and keys_got == keys and all(type(k) is int for k in keys_got)
            assert kw_got == kw and all(type(kw_got[n]) is type(v) for n, v in kw.items())
            both_channels(outs, VOICES)
            _, want_p, want_r = p.result(x, fs_got, keys_got)
            assert np.array_equal(period, want_p) and np.array_equal(ratio, want_r)
    # a recording shorter than the tracker's window: the row is frame_len + ceil(fs / 100) samples
    p = stub()
    outs = offline.pv_autotune(VOICES[:1], 44100.0, processor=p)
    assert p.calls[0][0][0].shape == (1, 1024 + 441) and p.calls[0][0][2] == [12] and isinstance(outs, list) and outs[0].shape == (2, 1)
    raises("pvtune --formant: 1024-point frames expected (the formant kernels are not built for 2048)", offline.pv_autotune, VOICES, 44100.0, formant=0.0,
           F=2048, hop=512, locked=True, processor=stub())
    raises(LOCK_2K_MSG, offline.pv_autotune, VOICES, 44100.0, F=2048, hop=512, locked=True, processor=stub())


def test_pv_autotune_stream():
    def stub(N=1024):
        return _OneShot(tune_result(lambda x: (x.shape[1] // N, x.shape[0])))
    for fs, N, hop, F in ((44100, 1024, 256, 1024), (8000.0, 64, 128, 2048), (51200.0, 100, 256, 1024)):
        lat = 1024 - int(np.gcd(N, hop))
        T = -(-(2500 + lat) // N) * N
        for extra, kw, key, keys in tune_common(offline.pv_autotune_stream, stub):
            p = _OneShot(lambda x, fs, keys: (np.roll(x, lat, axis=1),) + tune_result(lambda x: (x.shape[1] // N, x.shape[0]))(x, fs, keys)[1:])
            outs, period, ratio = offline.pv_autotune_stream(VOICES, fs, key=key, N=N, hop=hop, F=F, processor=p, with_track=True, **extra)
            ((x, fs_got, keys_got), kw_got), = p.calls
            is_batch(x, T)
            assert fs_got == float(fs) and type(fs_got) is float and keys_got == keys and all(type(k) is int for k in keys_got)
            assert kw_got == kw and all(type(kw_got[n]) is type(v) for n, v in kw.items())
            both_channels(outs, VOICES)                       # the shifter's latency is off the front
            assert period.shape == ratio.shape == (T // N, S) and np.array_equal(period, p.result(x, fs_got, keys_got)[1])
    p = stub()
    assert isinstance(offline.pv_autotune_stream(VOICES, 44100.0, processor=p), list)
    for bad in (dict(N=0), dict(F=512), dict(F=4096, hold=-1)):
        raises("pvtune --stream: a block of at least one sample and a tracker frame of 1024 or 2048 expected", offline.pv_autotune_stream, VOICES, 44100.0,
               processor=stub(), **bad)
    for bad in (dict(hold=-1), dict(hold=(1 << 20) + 1), dict(glide=0.0), dict(glide=1.5), dict(glide=float("nan"))):
        raises("pvtune --stream: 0 <= hold <= 2^20 blocks and 0 < glide <= 1 expected", offline.pv_autotune_stream, VOICES, 44100.0, processor=stub(), **bad)
