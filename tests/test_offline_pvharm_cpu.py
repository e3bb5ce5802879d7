"""What the harmonize flow of vocoderproject_amd.offline hands to its processor and gives back, every ValueError it raises, and its
command line from WAV files to WAV files.  The processors are recording stand-ins; the expected arrays are worked out here from the
flow's documented arithmetic, not taken from the module."""
import numpy as np
import pytest

from vocoderproject_amd import offline

LENS = (1, 300, 2500)
VOICES = [((np.arange(n) % 97 + 1) / 128.0 * (-1) ** s).astype(np.float32) for s, n in enumerate(LENS)]
S = len(VOICES)


def raises(msg, fn, *a, **kw):
    with pytest.raises(ValueError) as e:
        fn(*a, **kw)
    assert str(e.value) == msg, (str(e.value), msg)


def packed(T):
    x = np.zeros((S, T), np.float32)
    for s, (r, n) in enumerate(zip(VOICES, LENS)):
        x[s, :n] = r[:n]
    return x


class _OneShot:
    def __init__(self):
        self.calls = []

    def run(self, x, semitones, gains, dry):
        self.calls.append((x.copy(), np.array(semitones), np.array(gains), dry))
        return (0.5 * x).astype(np.float32)


class _Stream:
    def __init__(self, latency):
        self.calls, self.latency = [], latency

    def run(self, x, **kw):
        self.calls.append((x.copy(), kw))
        return (-x).astype(np.float32)


def both_channels(outs, rows):
    assert len(outs) == S
    for s, o in enumerate(outs):
        assert o.dtype == np.float32 and o.shape == (2, LENS[s]) and o.flags.c_contiguous, (s, o.dtype, o.shape)
        assert np.array_equal(o[0], rows[s][:LENS[s]]) and np.array_equal(o[1], o[0]), s


def test_pv_harmonize_batch_builds_the_table_per_stream_voice_and_frame():
    for hop, T in ((256, 1024 + 10 * 256), (128, 1024 + 20 * 128)):                # 1024 + ceil(2500 / hop) hop
        nF = (T - 1024) // hop + 1
        for iv, gains, wantg in (((4, 7, -5), None, [1.0, 1.0, 1.0]), ([12.0], [0.5], [0.5]), ((-12, 0.37, 3, 7), (1, -4, 0, 4), [1.0, -4.0, 0.0, 4.0])):
            for dry, wantd in ((1.0, [1.0] * 3), ([0, 0.5, -4], [0.0, 0.5, -4.0])):
                p = _OneShot()
                outs = offline.pv_harmonize(VOICES, iv, gains=gains, dry=dry, hop=hop, processor=p)
                (x, st, g, d), = p.calls
                assert x.dtype == np.float32 and np.array_equal(x, packed(T))
                assert st.dtype == np.float64 and st.shape == (S, len(iv), nF)
                for v, want in enumerate(iv):
                    assert np.all(st[:, v, :] == float(want))
                assert g.dtype == np.float64 and g.shape == (S, len(iv)) and np.all(g == np.array(wantg)[None, :])
                assert d == wantd and all(type(v) is float for v in d)
                both_channels(outs, 0.5 * x)
    p = _OneShot()
    offline.pv_harmonize(VOICES, (4, 7), processor=p)
    assert p.calls[0][3] == [1.0] * 3                                               # the dry signal is in by default


def test_pv_harmonize_stream_builds_the_table_per_block_stream_and_voice():
    for N, hop, lat in ((256, 128, 896), (100, 256, 1020)):
        p = _Stream(lat)
        outs = offline.pv_harmonize(VOICES, (4, -5), gains=(1, 0.7), dry=0.25, N=N, hop=hop, stream=True, blocks_per_call=3, processor=p)
        (x, kw), = p.calls
        nb = -(-(2500 + lat) // N)
        assert x.shape == (S, 2500) and np.array_equal(x, packed(2500))             # (run's output is aligned with its input: the latency is off)
        assert sorted(kw) == ["blocks_per_call", "dry", "gains", "semitones"] and kw["blocks_per_call"] == 3 and kw["dry"] == [0.25] * 3
        assert kw["semitones"].shape == (nb, S, 2) and np.all(kw["semitones"][..., 0] == 4.0) and np.all(kw["semitones"][..., 1] == -5.0)
        assert kw["gains"].shape == (S, 2) and np.all(kw["gains"] == np.array([1.0, 0.7]))
        both_channels(outs, -x)


def test_pv_harmonize_refuses():
    raises("no recordings", offline.pv_harmonize, [], (4,), processor=_OneShot())
    for iv in ((), (1, 2, 3, 4, 5), 4.0):
        raises("voices: 1 to 4 intervals expected", offline.pv_harmonize, VOICES, iv, processor=_OneShot())
    for iv in ((4, 12.5), (-13,), (float("nan"),)):
        raises("voices: intervals within +-12 semitones expected", offline.pv_harmonize, VOICES, iv, processor=_OneShot())
    raises("gains: one gain per voice expected", offline.pv_harmonize, VOICES, (4, 7), gains=(1,), processor=_OneShot())
    for g in ((1, 4.5), (float("nan"), 1), (-5, 0)):
        raises("gains: values within [-4, 4] expected", offline.pv_harmonize, VOICES, (4, 7), gains=g, processor=_OneShot())
    raises("dry: one value per recording expected", offline.pv_harmonize, VOICES, (4,), dry=[1.0, 0.5], processor=_OneShot())
    for dry in (4.5, float("nan"), [0, 1, -5]):
        for stream in (False, True):
            raises("dry: values within [-4, 4] expected", offline.pv_harmonize, VOICES, (4,), dry=dry, stream=stream, processor=_Stream(896))
    raises("harmonize: 1024-point frames expected (the harmonizer kernels are not built for 2048)", offline.pv_harmonize, VOICES, (4,), F=2048, hop=512,
           processor=_OneShot())
    with pytest.raises(ValueError, match=r"voice 1: expected a mono signal, got shape \(2, 5\)"):
        offline.pv_harmonize([VOICES[0], np.zeros((2, 5), np.float32), VOICES[2]], (4,), processor=_OneShot())


def test_command_line(tmp_path, monkeypatch):
    fs = 22050
    a, b, car = (str(tmp_path / n) for n in ("a.wav", "b.wav", "car.wav"))
    ya = 0.25 * np.sin(np.arange(3000) * 0.05)
    yb = 0.25 * np.sin(np.arange(1200) * 0.11)
    offline.write_wav(a, fs, ya)
    offline.write_wav(b, fs, yb)
    offline.write_wav(car, fs, yb)
    seen = []

    def fake(voices, intervals, **kw):
        seen.append((voices, intervals, kw))
        return [np.stack([0.5 * v, 0.5 * v]) for v in voices]
    monkeypatch.setattr(offline, "pv_harmonize", fake)
    out = str(tmp_path / "o")
    assert offline.main(["harmonize", a, b, "--voices", "4,7,-5", "--out-dir", out]) == 0
    voices, iv, kw = seen.pop()
    assert [v.shape for v in voices] == [(3000,), (1200,)] and iv == [4.0, 7.0, -5.0]
    assert kw == dict(gains=None, dry=1.0, hop=256, N=1024, stream=False, device=0)
    for name, v in (("a", voices[0]), ("b", voices[1])):
        fs_got, y = offline.read_wav(str(tmp_path / "o" / f"{name}_harmonize.wav"))
        assert fs_got == fs and y.shape == (2, v.size) and np.abs(y[0] - 0.5 * v).max() <= 1.0 / 32767.0 and np.array_equal(y[0], y[1])
    assert offline.main(["harmonize", a, "--voices=-12,12", "--gains", "1,0.7", "--dry", "0", "--stream", "--block", "256", "--hop", "128", "--out-dir", out]) == 0
    voices, iv, kw = seen.pop()
    assert iv == [-12.0, 12.0] and kw == dict(gains=[1.0, 0.7], dry=0.0, hop=128, N=256, stream=True, device=0)
    for bad, flag in ((["--formant"], "--formant"), (["--locked"], "--locked"), (["--locked", "--subbin"], "--locked"), (["--subbin"], "--subbin"),
                      (["--shift", "3"], "--shift"), (["--glide", "0.5"], "--glide"), (["--stretch", "1.5"], "--stretch"), (["--carrier", car], "--carrier"),
                      (["--track-csv"], "--track-csv"), (["--hold", "2"], "--hold")):
        with pytest.raises(SystemExit) as e:
            offline.main(["harmonize", a, "--voices", "4"] + bad + ["--out-dir", out])
        assert str(e.value) == f"{flag}: harmonize does not take it (its voices are peak-locked copies at the fixed intervals of --voices)", e.value
    with pytest.raises(SystemExit, match="harmonize needs --voices"):
        offline.main(["harmonize", a, "--out-dir", out])
    for bad in (["--voices", "4,x"], ["--voices", "4", "--gains", "1;2"]):
        with pytest.raises(SystemExit, match="--voices, --gains: comma-separated numbers expected"):
            offline.main(["harmonize", a] + bad + ["--out-dir", out])
    # the other flows refuse the new flags and keep their own messages
    for flow, extra in (("pvshift", ["--shift", "3"]), ("pvcross", ["--carrier", car]), ("stretch", ["--stretch", "2"])):
        with pytest.raises(SystemExit, match="--voices, --gains: harmonize takes them"):
            offline.main([flow, a] + extra + ["--voices", "4", "--out-dir", out])
    with pytest.raises(SystemExit, match="--formant: pvshift and pvtune take it"):
        offline.main(["stretch", a, "--stretch", "2", "--formant", "--out-dir", out])
    with pytest.raises(SystemExit) as e:
        offline.main(["pvcross", a, "--carrier", car, "--locked", "--out-dir", out])
    assert str(e.value) == "--locked: pvcross does not take it (the cross-synthesis moves neither pitch nor time)"
    assert not seen

    def refuse(voices, intervals, **kw):
        raise ValueError("voices: intervals within +-12 semitones expected")
    monkeypatch.setattr(offline, "pv_harmonize", refuse)
    with pytest.raises(SystemExit, match="voices: intervals within"):
        offline.main(["harmonize", a, "--voices", "13", "--out-dir", out])
