"""The offline front end of the streaming pitch tracker and correction (`python -m vocoderproject_amd.offline pvtune --stream`,
offline.pv_autotune_stream): argument parsing, block padding and latency, and the per-block CSV.  The DSP needs the GPU
(tests/test_gpu_pv_track_stream.py); here the processor is a stand-in that delays its input by the shifter's latency and returns a
made-up track, so that the plumbing around the hot path is what gets checked."""
import os

import numpy as np
import pytest

from vocoderproject_amd import offline


class _Stub:
    """_StreamTuneRunner's interface: the output is the input `lat` samples late, period b + 100 s on block b of stream s (0 on every third
    block), ratio 2^(1/12) where voiced."""

    def __init__(self, N, lat):
        self.N, self.lat, self.calls = N, lat, []

    def run(self, x, fs, keys):
        assert x.dtype == np.float32 and x.ndim == 2 and x.flags.c_contiguous and x.shape[1] % self.N == 0
        self.calls.append((x.copy(), fs, list(keys)))
        nb = x.shape[1] // self.N
        y = np.zeros_like(x)
        y[:, self.lat:] = x[:, :x.shape[1] - self.lat]
        period = np.array([[0 if b % 3 == 2 else b + 100 * s for s in range(x.shape[0])] for b in range(nb)], np.int32)
        return y, period, np.where(period > 0, 2.0 ** (1.0 / 12.0), 1.0)


def test_batch_is_padded_to_whole_blocks_behind_the_latency_and_trimmed_back():
    rng = np.random.default_rng(3)
    voices = [rng.normal(0, 0.1, n).astype(np.float32) for n in (5000, 300, 1, 2048)]
    for N, hop, lat in ((256, 256, 768), (1000, 256, 1016), (64, 128, 960)):
        assert offline.stream_tune_length(5000, N, hop) == (-(-(5000 + lat) // N) * N, lat)
        stub = _Stub(N, lat)
        outs, period, ratio = offline.pv_autotune_stream(voices, 44100.0, key=[0, 12, 7, 3], N=N, hop=hop, processor=stub, with_track=True)
        (x, fs, keys), = stub.calls
        T = offline.stream_tune_length(5000, N, hop)[0]
        assert x.shape == (4, T) and T % N == 0 and T - N < 5000 + lat <= T and fs == 44100.0 and keys == [0, 12, 7, 3]
        for s, v in enumerate(voices):
            assert np.array_equal(x[s, :v.size], v) and np.all(x[s, v.size:] == 0)
            assert outs[s].shape == (2, v.size) and np.array_equal(outs[s][0], v) and np.array_equal(outs[s][1], v)    # the latency is off
        assert period.shape == ratio.shape == (T // N, 4)
    assert offline.pv_autotune_stream(voices, 44100.0, N=256, processor=_Stub(256, 768))[0].shape == (2, 5000)      # without the track


def test_arguments_are_checked_before_the_processor_is_touched():
    v = [np.zeros(3000, np.float32)] * 2
    for kw in (dict(key=[0]), dict(key=13), dict(key=-1), dict(N=0), dict(F=512), dict(hold=-1), dict(hold=(1 << 20) + 1), dict(glide=0.0),
               dict(glide=1.5), dict(glide=float("nan"))):
        with pytest.raises(ValueError):
            offline.pv_autotune_stream(v, 44100.0, processor=None, **kw)
    for fs in (7999.0, 96000.0):
        with pytest.raises(ValueError):
            offline.pv_autotune_stream(v, fs, processor=None)
    with pytest.raises(ValueError):
        offline.pv_autotune_stream([], 44100.0, processor=_Stub(1024, 768))
    with pytest.raises(ValueError):
        offline.pv_autotune_stream([np.zeros((2, 3000), np.float32)], 44100.0, processor=_Stub(1024, 768))


def test_command_line(tmp_path, monkeypatch):
    a, b = str(tmp_path / "a.wav"), str(tmp_path / "b.wav")
    t = np.arange(6000) / 22050.0
    offline.write_wav(a, 22050, 0.5 * np.sin(2 * np.pi * 220.0 * t))
    offline.write_wav(b, 22050, 0.5 * np.sin(2 * np.pi * 330.0 * t[:2500]))
    seen, real = {}, offline.pv_autotune_stream

    def fake(voices, fs, key=12, N=1024, hop=256, F=1024, hold=0, glide=1.0, device=0, processor=None, with_track=False):
        seen.update(fs=fs, key=key, N=N, hop=hop, F=F, hold=hold, glide=glide, lens=[v.size for v in voices], with_track=with_track)
        return real(voices, fs, key=key, N=N, hop=hop, F=F, hold=hold, glide=glide, processor=_Stub(N, offline.stream_tune_length(1, N, hop)[1]),
                    with_track=with_track)

    def batch(*args, **kw):
        raise AssertionError("--stream must not take the one-shot path")

    monkeypatch.setattr(offline, "pv_autotune_stream", fake)
    monkeypatch.setattr(offline, "pv_autotune", batch)
    out = tmp_path / "o"
    assert offline.main(["pvtune", a, b, "--stream", "--key", "0", "--block", "200", "--hop", "128", "--hold", "5", "--glide", "0.5", "--frame", "2048",
                         "--out-dir", str(out), "--track-csv"]) == 0
    assert seen == dict(fs=22050, key=0, N=200, hop=128, F=2048, hold=5, glide=0.5, lens=[6000, 2500], with_track=True)
    for s, (name, n) in enumerate((("a", 6000), ("b", 2500))):
        fs, y = offline.read_wav(str(out / f"{name}_pvtune.wav"))
        assert fs == 22050 and y.shape == (2, n)
        rows = open(str(out / f"{name}_pvtune.csv")).read().splitlines()
        assert rows[0] == "time_s,period,semitones" and len(rows) - 1 == -(-n // 200)               # the blocks that start inside it
        cells = [r.split(",") for r in rows[1:]]
        assert [int(c[1]) for c in cells] == [0 if k % 3 == 2 else k + 100 * s for k in range(len(cells))]   # this recording's column of the table
        assert np.allclose([float(c[0]) for c in cells], np.arange(len(cells)) * 200 / 22050.0, atol=1e-6)
    assert offline.main(["pvtune", a, "--stream", "--out-dir", str(tmp_path / "p")]) == 0                # the defaults
    assert (seen["N"], seen["hold"], seen["glide"], seen["key"]) == (1024, 0, 1.0, 12) and not os.path.exists(str(tmp_path / "p" / "a_pvtune.csv"))
    for bad in (["--glide", "2"], ["--glide", "1:2"], ["--hold", "-1"], ["--key", "13"]):
        with pytest.raises(SystemExit):
            offline.main(["pvtune", a, "--stream", "--out-dir", str(tmp_path / "q")] + bad)
