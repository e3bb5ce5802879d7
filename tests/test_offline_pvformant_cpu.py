"""The offline front end of the formant-preserving pitch shift (`python -m vocoderproject_amd.offline pvshift|pvtune ... --formant [ST]
--lifter N`, offline.pv_shift_formant and the formant arguments of pv_glide, pv_autotune, pv_autotune_stream): the new flags parse and
reach the calls, batching and padding.  The DSP needs the GPU (tests/test_gpu_pv_formant.py); here the processors are stand-ins that
return their input, so that the plumbing around the hot path is what gets checked."""
import numpy as np
import pytest

from vocoderproject_amd import offline


class _Batch:
    """_FormantShiftRunner's interface."""

    def __init__(self):
        self.calls = []

    def run(self, x, semitones, formant, lifter):
        assert x.dtype == np.float32 and x.ndim == 2 and x.flags.c_contiguous
        self.calls.append((x.copy(), list(semitones), formant, lifter))
        return x.copy()


class _Stream:
    """PhaseVocoderStream's interface as pv_glide and pv_shift_formant use it."""
    latency = 768

    def __init__(self):
        self.calls = []

    def run(self, x, blocks_per_call=8, curve=None, **kw):
        self.calls.append((x.copy(), blocks_per_call, np.array(curve), kw))
        return x.copy()


class _Tune:
    """_AutotuneRunner's / _StreamTuneRunner's interface; rows: frames (batch) or None (stream: blocks of 1024)."""

    def __init__(self, stream=False):
        self.calls, self.stream = [], stream

    def run(self, x, fs, keys, **kw):
        self.calls.append((x.shape, fs, list(keys), kw))
        n = x.shape[1] // 1024 if self.stream else (x.shape[1] - 1024) // 256 + 1
        shape = (n, x.shape[0]) if self.stream else (x.shape[0], n)
        return x.copy(), np.zeros(shape, np.int32), np.ones(shape)


VOICES = [np.random.default_rng(s).normal(0, 0.1, n).astype(np.float32) for s, n in enumerate((5000, 300, 2048))]


def test_batch_shift_is_padded_under_the_full_overlap_and_trimmed_back():
    stub = _Batch()
    outs = offline.pv_shift_formant(VOICES, [3.0, -2.0, 12.0], formant=-4.0, lifter=16, hop=128, processor=stub)
    (x, semis, formant, lifter), = stub.calls
    assert x.shape == (3, 1024 + 40 * 128) and semis == [3.0, -2.0, 12.0] and formant == -4.0 and lifter == 16
    for s, v in enumerate(VOICES):
        assert np.array_equal(x[s, :v.size], v) and np.all(x[s, v.size:] == 0)
        assert outs[s].shape == (2, v.size) and np.array_equal(outs[s][0], v) and np.array_equal(outs[s][1], v)
    stub = _Batch()
    offline.pv_shift_formant(VOICES, 7.0, processor=stub)                      # one interval for all; preservation and lifter 32 by default
    assert stub.calls[0][1:] == ([7.0] * 3, 0.0, 32)


def test_streamed_shift_and_glide_pass_the_formant_arguments_to_run():
    stub = _Stream()
    outs = offline.pv_shift_formant(VOICES, [3.0, -2.0, 12.0], formant=2.0, lifter=64, N=256, stream=True, processor=stub)
    (x, k, curve, kw), = stub.calls
    assert x.shape == (3, 5000) and curve.tolist() == [[3.0, -2.0, 12.0]] and kw == dict(formant_semitones=2.0, lifter=64)
    assert [o.shape for o in outs] == [(2, 5000), (2, 300), (2, 2048)]
    stub = _Stream()
    offline.pv_glide(VOICES, -12.0, 12.0, N=1024, processor=stub, formant=0.0, lifter=8)
    assert stub.calls[0][3] == dict(formant_semitones=0.0, lifter=8) and stub.calls[0][2].shape == (6, 3)
    stub = _Stream()
    offline.pv_glide(VOICES, -12.0, 12.0, N=1024, processor=stub)              # without --formant: the call as it was
    assert stub.calls[0][3] == {}


def test_autotune_passes_the_formant_arguments_only_when_given():
    for fn, stream in ((offline.pv_autotune, False), (offline.pv_autotune_stream, True)):
        stub = _Tune(stream)
        fn(VOICES, 44100.0, key=3, processor=stub)
        assert stub.calls[0][3] == {}
        stub = _Tune(stream)
        outs = fn(VOICES, 44100.0, key=3, processor=stub, formant=0.0)
        assert stub.calls[0][3] == dict(formant=0.0, lifter=32) and stub.calls[0][2] == [3, 3, 3] and outs[0].shape == (2, 5000)
        stub = _Tune(stream)
        fn(VOICES, 44100.0, processor=stub, formant=-5.0, lifter=4)
        assert stub.calls[0][3] == dict(formant=-5.0, lifter=4)


def test_arguments_are_checked_before_the_processor_is_touched():
    for kw in (dict(formant=12.5), dict(formant=-13.0), dict(lifter=3), dict(lifter=65)):
        with pytest.raises(ValueError):
            offline.pv_shift_formant(VOICES, 0.0, processor=None, **kw)
        with pytest.raises(ValueError):
            offline.pv_autotune(VOICES, 44100.0, processor=None, **dict(dict(formant=0.0), **kw))
        with pytest.raises(ValueError):
            offline.pv_autotune_stream(VOICES, 44100.0, processor=None, **dict(dict(formant=0.0), **kw))
        with pytest.raises(ValueError):
            offline.pv_glide(VOICES, 0.0, 1.0, processor=_Stream(), **dict(dict(formant=0.0), **kw))
    for kw in (dict(shift=13.0), dict(shift=[0.0])):
        with pytest.raises(ValueError):
            offline.pv_shift_formant(VOICES, kw["shift"], processor=None)
    with pytest.raises(ValueError):
        offline.pv_shift_formant([], 0.0, processor=_Batch())
    with pytest.raises(ValueError):
        offline.pv_autotune(VOICES, 44100.0, F=2048, hop=512, formant=0.0, processor=None)    # the formant kernels are 1024-point


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
    spy("pv_shift_formant", lambda kw: _Stream() if kw.get("stream") else _Batch())
    spy("pv_glide", lambda kw: _Stream())
    spy("pv_autotune", lambda kw: _Tune(False))
    spy("pv_autotune_stream", lambda kw: _Tune(True))
    monkeypatch.setattr(offline, "pv_shift", lambda *a_, **k: pytest.fail("pvshift --formant must not take the plain path"))
    out = str(tmp_path / "o")
    assert offline.main(["pvshift", a, b, "--shift", "5", "--formant", "--out-dir", out]) == 0
    assert seen[-1] == ("pv_shift_formant", (5.0,), dict(N=1024, hop=256, stream=False, formant=0.0, lifter=32))       # no value: preservation
    assert offline.read_wav(str(tmp_path / "o" / "b_pvshift.wav"))[1].shape == (2, 2500)
    assert offline.main(["pvshift", a, "--shift", "-7", "--formant", "-3.5", "--lifter", "12", "--stream", "--hop", "128", "--block", "512", "--out-dir", out]) == 0
    assert seen[-1] == ("pv_shift_formant", (-7.0,), dict(N=512, hop=128, stream=True, formant=-3.5, lifter=12))
    assert offline.main(["pvshift", a, "--glide", "-12:12", "--formant", "2", "--out-dir", out]) == 0
    assert seen[-1] == ("pv_glide", (-12.0, 12.0), dict(N=1024, hop=256, formant=2.0, lifter=32))
    assert offline.main(["pvtune", a, b, "--key", "0", "--formant", "--lifter", "48", "--out-dir", out]) == 0
    assert seen[-1] == ("pv_autotune", (22050,), dict(key=0, F=1024, hop=256, with_track=True, formant=0.0, lifter=48))
    assert offline.main(["pvtune", a, "--stream", "--formant", "1.5", "--out-dir", out]) == 0
    assert seen[-1][0] == "pv_autotune_stream" and seen[-1][2]["formant"] == 1.5 and seen[-1][2]["lifter"] == 32
    assert offline.main(["pvtune", a, "--out-dir", out]) == 0                   # without the flag: the calls as they were
    assert "formant" not in seen[-1][2] and "lifter" not in seen[-1][2]
    for bad in (["pvshift", a, "--shift", "1", "--formant", "13"], ["pvshift", a, "--shift", "1", "--formant", "--lifter", "2"],
                ["pvtune", a, "--formant", "--frame", "2048", "--hop", "512"], ["pitch", a, "--formant"]):
        with pytest.raises(SystemExit):
            offline.main(bad + ["--out-dir", out])
