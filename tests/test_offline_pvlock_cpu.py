"""The offline front end of the peak-locked pitch shift (`python -m vocoderproject_amd.offline pvshift --locked (--shift | --glide)`,
`pvtune --locked [--stream]`; offline.pv_shift_locked and the `locked` argument of pv_glide, pv_autotune, pv_autotune_stream): the flag
parses and reaches the calls, and without it the recorded calls are the ones made before it existed.  The DSP needs the GPU
(tests/test_gpu_pv_lock.py); here the processors are stand-ins that return their input."""
import numpy as np
import pytest

from vocoderproject_amd import offline


class _Stream:
    """PhaseVocoderStream's interface as pv_glide and pv_shift_locked use it."""
    latency = 768

    def __init__(self):
        self.calls = []

    def run(self, x, blocks_per_call=8, curve=None, **kw):
        assert x.dtype == np.float32 and x.ndim == 2
        self.calls.append((x.copy(), blocks_per_call, np.array(curve), kw))
        return x.copy()


class _Tune:
    """_AutotuneRunner's / _StreamTuneRunner's interface."""

    def __init__(self, stream=False):
        self.calls, self.stream = [], stream

    def run(self, x, fs, keys, **kw):
        self.calls.append((x.shape, fs, list(keys), kw))
        n = x.shape[1] // 1024 if self.stream else (x.shape[1] - 1024) // 256 + 1
        shape = (n, x.shape[0]) if self.stream else (x.shape[0], n)
        return x.copy(), np.zeros(shape, np.int32), np.ones(shape)


VOICES = [np.random.default_rng(s).normal(0, 0.1, n).astype(np.float32) for s, n in enumerate((5000, 300, 2048))]


def test_locked_shift_streams_a_constant_curve():
    stub = _Stream()
    outs = offline.pv_shift_locked(VOICES, [3.0, -2.0, 12.0], N=256, processor=stub)
    (x, k, curve, kw), = stub.calls
    assert x.shape == (3, 5000) and k == 16 and curve.tolist() == [[3.0, -2.0, 12.0]] and kw == dict(locked=True)
    for s, v in enumerate(VOICES):
        assert np.array_equal(x[s, :v.size], v) and np.all(x[s, v.size:] == 0)
        assert outs[s].shape == (2, v.size) and np.array_equal(outs[s][0], v) and np.array_equal(outs[s][1], v)
    stub = _Stream()
    offline.pv_shift_locked(VOICES, 7.0, processor=stub)
    assert stub.calls[0][2].tolist() == [[7.0] * 3]


def test_glide_and_autotune_pass_locked_only_when_given():
    stub = _Stream()
    offline.pv_glide(VOICES, -12.0, 12.0, N=1024, processor=stub, locked=True)
    assert stub.calls[0][3] == dict(locked=True) and stub.calls[0][2].shape == (6, 3)
    stub = _Stream()
    offline.pv_glide(VOICES, -12.0, 12.0, N=1024, processor=stub)              # without the flag: the call as it was
    assert stub.calls[0][3] == {}
    for fn, stream in ((offline.pv_autotune, False), (offline.pv_autotune_stream, True)):
        stub = _Tune(stream)
        fn(VOICES, 44100.0, key=3, processor=stub)
        assert stub.calls[0][3] == {}
        stub = _Tune(stream)
        outs = fn(VOICES, 44100.0, key=3, processor=stub, locked=True)
        assert stub.calls[0][3] == dict(locked=True) and stub.calls[0][2] == [3, 3, 3] and outs[0].shape == (2, 5000)


def test_arguments_are_checked_before_the_processor_is_touched():
    for shift in (13.0, [0.0], [0.0, 1.0, -12.5]):
        with pytest.raises(ValueError):
            offline.pv_shift_locked(VOICES, shift, processor=None)
    with pytest.raises(ValueError):
        offline.pv_shift_locked([], 0.0, processor=_Stream())
    with pytest.raises(ValueError):
        offline.pv_glide(VOICES, 0.0, 1.0, processor=None, locked=True, formant=0.0)
    with pytest.raises(ValueError):
        offline.pv_autotune(VOICES, 44100.0, processor=None, locked=True, formant=0.0)
    with pytest.raises(ValueError):
        offline.pv_autotune_stream(VOICES, 44100.0, processor=None, locked=True, formant=0.0)
    with pytest.raises(ValueError):
        offline.pv_autotune(VOICES, 44100.0, F=2048, hop=512, locked=True, processor=None)    # the locked kernels are 1024-point


def test_command_line(tmp_path, monkeypatch):
    a, b = str(tmp_path / "a.wav"), str(tmp_path / "b.wav")
    t = np.arange(6000) / 22050.0
    offline.write_wav(a, 22050, 0.5 * np.sin(2 * np.pi * 220.0 * t))
    offline.write_wav(b, 22050, 0.5 * np.sin(2 * np.pi * 330.0 * t[:2500]))
    seen = []

    def spy(name, stub_of):
        real = getattr(offline, name)

        def fake(voices, *args, **kw):
            seen.append((name, args, {k: v for k, v in kw.items() if k != "device"}))
            kw.pop("device", None)
            return real(voices, *args, processor=stub_of(kw), **kw)
        monkeypatch.setattr(offline, name, fake)
    spy("pv_shift_locked", lambda kw: _Stream())
    spy("pv_glide", lambda kw: _Stream())
    spy("pv_autotune", lambda kw: _Tune(False))
    spy("pv_autotune_stream", lambda kw: _Tune(True))
    plain = []
    monkeypatch.setattr(offline, "pv_shift", lambda voices, shift, **kw: plain.append((shift, kw)) or [np.stack([v, v]) for v in voices])
    out = str(tmp_path / "o")
    assert offline.main(["pvshift", a, b, "--shift", "5", "--locked", "--out-dir", out]) == 0
    assert seen[-1] == ("pv_shift_locked", (5.0,), dict(N=1024, hop=256)) and not plain
    assert offline.read_wav(str(tmp_path / "o" / "b_pvshift.wav"))[1].shape == (2, 2500)
    assert offline.main(["pvshift", a, "--glide", "-12:12", "--locked", "--hop", "128", "--out-dir", out]) == 0
    assert seen[-1] == ("pv_glide", (-12.0, 12.0), dict(N=1024, hop=128, locked=True))
    assert offline.main(["pvtune", a, b, "--key", "0", "--locked", "--out-dir", out]) == 0
    assert seen[-1] == ("pv_autotune", (22050,), dict(key=0, F=1024, hop=256, with_track=True, locked=True))
    assert offline.main(["pvtune", a, "--stream", "--locked", "--out-dir", out]) == 0
    assert seen[-1][0] == "pv_autotune_stream" and seen[-1][2]["locked"] is True
    # without the flag: the calls as they were
    n = len(seen)
    assert offline.main(["pvshift", a, "--shift", "5", "--out-dir", out]) == 0
    assert len(seen) == n and plain == [(5.0, dict(N=1024, hop=256, device=0))]
    assert offline.main(["pvshift", a, "--glide", "-12:12", "--out-dir", out]) == 0
    assert seen[-1] == ("pv_glide", (-12.0, 12.0), dict(N=1024, hop=256))
    assert offline.main(["pvtune", a, "--out-dir", out]) == 0
    assert seen[-1] == ("pv_autotune", (22050,), dict(key=12, F=1024, hop=256, with_track=True))
    assert offline.main(["pvtune", a, "--stream", "--out-dir", out]) == 0
    assert "locked" not in seen[-1][2]
    for bad in (["pvshift", a, "--shift", "1", "--locked", "--formant"], ["pvtune", a, "--locked", "--formant", "2"],
                ["pvtune", a, "--locked", "--frame", "2048", "--hop", "512"], ["pitch", a, "--locked"], ["pvshift", a, "--shift", "13", "--locked"]):
        with pytest.raises(SystemExit):
            offline.main(bad + ["--out-dir", out])
