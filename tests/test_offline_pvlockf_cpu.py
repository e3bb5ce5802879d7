"""The offline front end of the peak-locked pitch shift with sub-bin region offsets (`python -m vocoderproject_amd.offline pvshift
--locked --subbin (--shift | --glide) [--stream]`, `pvtune --locked --subbin [--stream]`; the `subbin` argument of offline.pv_shift_locked,
pv_glide, pv_autotune, pv_autotune_stream): the flag parses and reaches the calls as locked=True, subbin=True, every refusal comes with
its own message before a processor is made, and without the flag the recorded calls carry exactly the keywords they carried before it
existed.  The DSP needs the GPU (tests/test_gpu_pv_lockf.py); here the processors are stand-ins that return their input."""
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
BOTH = dict(locked=True, subbin=True)


def _no_processor(monkeypatch):
    """Any attempt to make a real processor fails the test."""
    def boom(*a, **k):
        raise AssertionError("a processor was made")
    for name in ("_stream", "_AutotuneRunner", "_StreamTuneRunner", "_StretchRunner", "_CrossRunner"):
        monkeypatch.setattr(offline, name, boom)


def test_the_flows_pass_locked_and_subbin():
    stub = _Stream()
    outs = offline.pv_shift_locked(VOICES, [3.0, -2.0, 12.0], N=256, processor=stub, subbin=True)
    (x, k, curve, kw), = stub.calls
    assert x.shape == (3, 5000) and k == 16 and curve.tolist() == [[3.0, -2.0, 12.0]] and kw == BOTH
    for s, v in enumerate(VOICES):
        assert outs[s].shape == (2, v.size) and np.array_equal(outs[s][0], v)
    stub = _Stream()
    offline.pv_glide(VOICES, -12.0, 12.0, N=1024, processor=stub, locked=True, subbin=True)
    assert stub.calls[0][3] == BOTH and stub.calls[0][2].shape == (6, 3)
    for fn, stream in ((offline.pv_autotune, False), (offline.pv_autotune_stream, True)):
        stub = _Tune(stream)
        outs = fn(VOICES, 44100.0, key=3, processor=stub, locked=True, subbin=True)
        assert stub.calls[0][3] == BOTH and stub.calls[0][2] == [3, 3, 3] and outs[0].shape == (2, 5000)


def test_flows_without_the_flag_pass_exactly_the_keywords_they_passed_before():
    stub = _Stream()
    offline.pv_shift_locked(VOICES, 7.0, processor=stub)
    assert stub.calls[0][3] == dict(locked=True)
    stub = _Stream()
    offline.pv_glide(VOICES, -12.0, 12.0, processor=stub, locked=True)
    assert stub.calls[0][3] == dict(locked=True)
    stub = _Stream()
    offline.pv_glide(VOICES, -12.0, 12.0, processor=stub)
    assert stub.calls[0][3] == {}
    stub = _Stream()
    offline.pv_glide(VOICES, -12.0, 12.0, processor=stub, formant=0.0)
    assert stub.calls[0][3] == dict(formant_semitones=0.0, lifter=32)
    for fn, stream in ((offline.pv_autotune, False), (offline.pv_autotune_stream, True)):
        stub = _Tune(stream)
        fn(VOICES, 44100.0, processor=stub)
        assert stub.calls[0][3] == {}
        stub = _Tune(stream)
        fn(VOICES, 44100.0, processor=stub, locked=True)
        assert stub.calls[0][3] == dict(locked=True)
    assert offline._mode_kw(None, 0, False) == {} and offline._mode_kw(None, 0, True) == dict(locked=True)
    assert offline._mode_kw(None, 0, True, subbin=True) == BOTH


def test_subbin_without_locked_is_refused_before_a_processor_is_made(monkeypatch):
    _no_processor(monkeypatch)
    for call in (lambda: offline.pv_glide(VOICES, 0.0, 1.0, subbin=True),
                 lambda: offline.pv_autotune(VOICES, 44100.0, subbin=True),
                 lambda: offline.pv_autotune_stream(VOICES, 44100.0, subbin=True)):
        with pytest.raises(ValueError, match="--subbin: valid only together with --locked"):
            call()
    # with a formant interval the locked / formant exclusion and its message win, unchanged
    for call in (lambda: offline.pv_glide(VOICES, 0.0, 1.0, locked=True, subbin=True, formant=0.0),
                 lambda: offline.pv_autotune(VOICES, 44100.0, locked=True, subbin=True, formant=0.0),
                 lambda: offline.pv_autotune_stream(VOICES, 44100.0, locked=True, subbin=True, formant=0.0)):
        with pytest.raises(ValueError, match="--locked and --formant exclude each other"):
            call()


def test_python_front_ends_refuse_subbin_without_locked_before_any_launch():
    """No GPU here: the refusal must come before the library is asked for anything."""
    from vocoderproject_amd import PhaseVocoderStream, StftRoundTrip
    ps = PhaseVocoderStream.__new__(PhaseVocoderStream)                                # (no handle: a call that reached the library would fail differently)
    ps.h = None
    with pytest.raises(ValueError, match="subbin=True needs locked=True"):
        ps.process_device(None, None, subbin=True)
    with pytest.raises(ValueError, match="subbin=True needs locked=True"):
        ps.run(np.zeros((1, 8), np.float32), subbin=True)
    with pytest.raises(ValueError, match="subbin=True needs locked=True"):
        ps.autotune_device(None, None, None, subbin=True)
    for call in (lambda: ps.process_device(None, None, locked=True, subbin=True, formant_semitones=0.0),
                 lambda: ps.run(np.zeros((1, 8), np.float32), locked=True, subbin=True, formant_semitones=0.0),
                 lambda: ps.autotune_device(None, None, None, locked=True, subbin=True, formant_semitones=0.0)):
        with pytest.raises(ValueError, match="locked and formant_semitones exclude each other"):
            call()
    import inspect
    for fn in (StftRoundTrip.pitch_shift_locked, StftRoundTrip.autotune, PhaseVocoderStream.process_device, PhaseVocoderStream.autotune_device,
               PhaseVocoderStream.run):
        assert inspect.signature(fn).parameters["subbin"].default is False, fn


def test_command_line(tmp_path, monkeypatch):
    a, b = str(tmp_path / "a.wav"), str(tmp_path / "b.wav")
    t = np.arange(6000) / 22050.0
    offline.write_wav(a, 22050, 0.5 * np.sin(2 * np.pi * 220.0 * t))
    offline.write_wav(b, 22050, 0.5 * np.sin(2 * np.pi * 330.0 * t[:2500]))
    seen, stubs = [], []

    def spy(name, stub_of):
        real = getattr(offline, name)

        def fake(voices, *args, **kw):
            seen.append((name, args, {k: v for k, v in kw.items() if k != "device"}))
            kw.pop("device", None)
            stubs.append(stub_of(kw))
            return real(voices, *args, processor=stubs[-1], **kw)
        monkeypatch.setattr(offline, name, fake)
    spy("pv_shift_locked", lambda kw: _Stream())
    spy("pv_glide", lambda kw: _Stream())
    spy("pv_autotune", lambda kw: _Tune(False))
    spy("pv_autotune_stream", lambda kw: _Tune(True))
    out = str(tmp_path / "o")
    assert offline.main(["pvshift", a, b, "--shift", "-12", "--locked", "--subbin", "--out-dir", out]) == 0
    assert seen[-1] == ("pv_shift_locked", (-12.0,), dict(N=1024, hop=256, subbin=True)) and stubs[-1].calls[0][3] == BOTH
    assert offline.read_wav(str(tmp_path / "o" / "b_pvshift.wav"))[1].shape == (2, 2500)
    assert offline.main(["pvshift", a, "--shift", "7", "--locked", "--subbin", "--stream", "--out-dir", out]) == 0
    assert seen[-1][0] == "pv_shift_locked" and stubs[-1].calls[0][3] == BOTH
    assert offline.main(["pvshift", a, "--glide", "-12:12", "--locked", "--subbin", "--hop", "128", "--out-dir", out]) == 0
    assert seen[-1] == ("pv_glide", (-12.0, 12.0), dict(N=1024, hop=128, locked=True, subbin=True)) and stubs[-1].calls[0][3] == BOTH
    assert offline.main(["pvtune", a, b, "--key", "0", "--locked", "--subbin", "--out-dir", out]) == 0
    assert seen[-1] == ("pv_autotune", (22050,), dict(key=0, F=1024, hop=256, with_track=True, locked=True, subbin=True))
    assert stubs[-1].calls[0][3] == BOTH
    assert offline.main(["pvtune", a, "--stream", "--locked", "--subbin", "--out-dir", out]) == 0
    assert seen[-1][0] == "pv_autotune_stream" and stubs[-1].calls[0][3] == BOTH
    # without the flag: the calls as they were
    assert offline.main(["pvshift", a, "--shift", "5", "--locked", "--out-dir", out]) == 0
    assert seen[-1] == ("pv_shift_locked", (5.0,), dict(N=1024, hop=256)) and stubs[-1].calls[0][3] == dict(locked=True)
    assert offline.main(["pvtune", a, "--locked", "--out-dir", out]) == 0
    assert seen[-1] == ("pv_autotune", (22050,), dict(key=12, F=1024, hop=256, with_track=True, locked=True))
    # the refusals, each with its own message, before a recording is read or a processor made
    n = len(seen)
    monkeypatch.setattr(offline, "read_wav", lambda f: (_ for _ in ()).throw(AssertionError("a recording was read")))
    for bad, text in ((["pvshift", a, "--shift", "1", "--subbin"], "--subbin: valid only together with --locked"),
                      (["pvshift", a, "--glide", "0:1", "--subbin"], "--subbin: valid only together with --locked"),
                      (["pvtune", a, "--subbin"], "--subbin: valid only together with --locked"),
                      (["pvtune", a, "--stream", "--subbin"], "--subbin: valid only together with --locked"),
                      (["stretch", a, "--stretch", "1.5", "--locked", "--subbin"], "--subbin: stretch does not take it"),
                      (["stretch", a, "--stretch", "1.5", "--subbin"], "--subbin: stretch does not take it"),
                      (["pvcross", a, "--carrier", b, "--subbin"], "--subbin: pvcross does not take it"),
                      (["pitch", a, "--subbin"], "--subbin: pvshift and pvtune take it"),
                      (["pvshift", a, "--shift", "1", "--locked", "--subbin", "--formant"], "--locked and --formant exclude each other")):
        with pytest.raises(SystemExit) as e:
            offline.main(bad + ["--out-dir", out])
        assert text in str(e.value), (bad, str(e.value))
    assert len(seen) == n
