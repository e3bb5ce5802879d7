"""CPU-side checks of `offline stretch --locked --transients [THR] [--span K]` and offline.pv_stretch(transients=, span=): the argument
rules, each refusal with its own message before a recording is read; the flow through a `processor=` stand-in built on the NumPy
definition (tests/pv_transient_reference.py) -- flux of the padded batch, every recording picked and planned against its own length, the
tables handed to run with reset= --; a file without onsets gives the two-anchor line; and without the flag the stretch flow passes exactly
what it passed before.  No GPU (the pick and the plan are the library's host functions)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pv_transient_cases as TC  # noqa: E402
import pv_transient_reference as TR  # noqa: E402
from vocoderproject_amd import offline  # noqa: E402

F = TC.F


class _Definition:
    """processor= built on the definition: flux(x) and run(x, pos, T, semitones, locked, reset) in NumPy; keeps what it was given."""

    def __init__(self, hop):
        self.hop, self.calls, self.fluxes = hop, [], 0

    def flux(self, x):
        self.fluxes += 1
        fm = [TR.onset_flux(r, F, self.hop) for r in x]
        return np.stack([a for a, _ in fm]), np.stack([b for _, b in fm])

    def run(self, x, pos, T, semitones, **kw):
        self.calls.append((x.shape, np.array(pos), T, semitones, {k: (np.array(v) if k == "reset" else v) for k, v in kw.items()}))
        reset = kw.get("reset")
        r = 2.0 ** (semitones / 12.0)
        return np.stack([TR.stretch_locked_reset_roundtrip(x[s], pos[s], T, r, None if reset is None else reset[s], F, self.hop) for s in range(len(x))]).astype(np.float32)


def _recordings(hop):
    """A burst recording, a shorter pluck recording, and a steady tone without onsets."""
    a = TC.bursts(F + 44 * hop + 5, [F + 6 * hop + 37, F + 27 * hop + 11], seed=1)
    b = TC.plucks(F + 30 * hop + 1, [F + 9 * hop + 3], seed=2)
    c = TC.LC.tone(F + 36 * hop, seed=3)
    return [a, b, c]


@pytest.mark.parametrize("hop,span", [(256, None), (512, 2)])
def test_every_recording_is_planned_against_its_own_length(hop, span):
    voices = _recordings(hop)
    p = _Definition(hop)
    stretch = [2.0, 0.75, 1.5]
    outs = offline.pv_stretch(voices, stretch, hop=hop, processor=p, locked=True, transients=0.2, span=span)
    assert p.fluxes == 1 and len(p.calls) == 1
    shape, pos, T, semis, kw = p.calls[0]
    assert shape == (3, max(len(v) for v in voices)) and semis == 0.0 and kw["locked"] is True and set(kw) == {"locked", "reset"}
    reset = kw["reset"]
    nF = (T - F) // hop + 1
    assert pos.shape == reset.shape == (3, nF) and pos.dtype == np.int32 and reset.dtype == np.uint8
    K = TR.default_span(F, hop) if span is None else span
    for s, (v, a) in enumerate(zip(voices, stretch)):
        flux, mass = TR.onset_flux(v, F, hop)                                             # the recording ALONE, its own length
        want_pos, want_reset = TR.plan_positions(TR.pick_onsets(flux, mass, 0.2), nF, hop, a, len(v), F, K)
        assert np.array_equal(pos[s], want_pos) and np.array_equal(reset[s], want_reset), s
        assert pos[s].max() <= len(v) - F                                                 # no frame reads the padding behind the recording
        assert outs[s].shape == (2, int(np.ceil(len(v) * a))) and np.array_equal(outs[s][0], outs[s][1])
    assert reset[0].sum() == 2 and reset[1].sum() == 1
    # the file without onsets: no flag, and the two-anchor line from (0, 0) to (nF - 1, base[nF - 1]) -- not pv_stretch's own table
    assert not reset[2].any()
    last = min(int(np.floor((nF - 1) * hop / stretch[2])), len(voices[2]) - F)
    assert list(pos[2]) == [(f * last) // (nF - 1) for f in range(nF)]
    # an attack leaves as it came: the span's output samples are the input's
    a0 = int(np.nonzero(reset[0])[0][0])
    t_out, t_in = (a0 + K) * hop, int(pos[0][a0 + K])
    seg = slice(F // 2 - hop // 2, F // 2 + hop // 2)
    assert np.abs(outs[0][0][t_out:t_out + F][seg] - voices[0][t_in:t_in + F][seg]).max() <= 1e-5 * max(1.0, np.abs(voices[0]).max())


def test_without_the_flag_the_flow_passes_what_it_passed_before():
    voices = _recordings(256)[:2]
    for kw, want in ((dict(), dict()), (dict(locked=True), dict(locked=True))):
        p = _Definition(256)
        offline.pv_stretch(voices, 1.5, shift=3.0, processor=p, **kw)
        assert p.fluxes == 0 and p.calls[0][3] == 3.0 and p.calls[0][4] == want
        nF = p.calls[0][1].shape[1]
        base = np.stack([np.minimum(np.floor(np.arange(nF) * 256 / 1.5), len(v) - F) for v in voices])
        assert np.array_equal(p.calls[0][1], base)


def test_the_python_front_end_refuses_bad_combinations_before_any_work():
    voices = _recordings(256)[:1]
    p = _Definition(256)
    for kw, text in ((dict(transients=0.2), "transients: valid only together with locked"),
                     (dict(locked=True, transients=1.5), "transients: a threshold within [0, 1] expected"),
                     (dict(locked=True, transients=-0.1), "transients: a threshold within [0, 1] expected"),
                     (dict(locked=True, transients=float("nan")), "transients: a threshold within [0, 1] expected"),
                     (dict(locked=True, transients=0.2, span=0), "span: 1 to 8 frames expected"),
                     (dict(locked=True, transients=0.2, span=9), "span: 1 to 8 frames expected"),
                     (dict(locked=True, span=2), "span: valid only together with transients"),
                     (dict(locked=True, transients=0.2, F=2048, hop=512), "--locked: 1024-point frames expected")):
        with pytest.raises(ValueError) as e:
            offline.pv_stretch(voices, 2.0, processor=p, **kw)
        assert text in str(e.value), (kw, str(e.value))
    assert p.fluxes == 0 and not p.calls


def test_command_line(tmp_path, monkeypatch):
    hop = 256
    a, b = str(tmp_path / "a.wav"), str(tmp_path / "b.wav")
    va, vb = _recordings(hop)[:2]
    offline.write_wav(a, 22050, va)
    offline.write_wav(b, 22050, vb)
    seen, stubs = [], []
    real = offline.pv_stretch

    def fake(voices, *args, **kw):
        seen.append((args, {k: v for k, v in kw.items() if k != "device"}))
        kw.pop("device", None)
        stubs.append(_Definition(kw.get("hop", 256)))
        return real(voices, *args, processor=stubs[-1], **kw)
    monkeypatch.setattr(offline, "pv_stretch", fake)
    out = str(tmp_path / "o")
    assert offline.main(["stretch", a, b, "--stretch", "2", "--locked", "--transients", "--out-dir", out]) == 0
    assert seen[-1] == ((2.0,), dict(shift=0.0, F=1024, hop=256, locked=True, transients=0.2, span=None))       # no value: the default threshold
    assert stubs[-1].fluxes == 1 and stubs[-1].calls[0][4]["reset"].any(axis=1).all()
    assert offline.read_wav(str(tmp_path / "o" / "b_stretch.wav"))[1].shape == (2, 2 * len(vb))
    assert offline.main(["stretch", a, "--stretch", "0.5", "--locked", "--transients", "0.35", "--span", "3", "--shift", "2", "--out-dir", out]) == 0
    assert seen[-1] == ((0.5,), dict(shift=2.0, F=1024, hop=256, locked=True, transients=0.35, span=3))
    assert offline.main(["stretch", a, "--stretch", "1.5", "--locked", "--out-dir", out]) == 0                   # without the flag: the call as it was
    assert seen[-1] == ((1.5,), dict(shift=0.0, F=1024, hop=256, locked=True)) and stubs[-1].fluxes == 0
    n = len(seen)
    monkeypatch.setattr(offline, "read_wav", lambda f: (_ for _ in ()).throw(AssertionError("a recording was read")))
    for bad, text in ((["stretch", a, "--stretch", "2", "--transients"], "--transients: valid only together with --locked"),
                      (["stretch", a, "--stretch", "2", "--transients", "0.3"], "--transients: valid only together with --locked"),
                      (["stretch", a, "--stretch", "2", "--locked", "--span", "2"], "--span: valid only together with --transients"),
                      (["pvshift", a, "--shift", "2", "--locked", "--transients"], "--transients: stretch takes it"),
                      (["pvtune", a, "--locked", "--transients", "0.2"], "--transients: stretch takes it")):
        with pytest.raises(SystemExit) as e:
            offline.main(bad + ["--out-dir", out])
        assert text in str(e.value), (bad, str(e.value))
    assert len(seen) == n
    # out-of-range values are the front end's to refuse, with its message
    monkeypatch.undo()
    for bad, text in ((["stretch", a, "--stretch", "2", "--locked", "--transients", "1.5"], "transients: a threshold within [0, 1] expected"),
                      (["stretch", a, "--stretch", "2", "--locked", "--transients", "--span", "9"], "span: 1 to 8 frames expected"),
                      (["stretch", a, "--stretch", "2", "--locked", "--transients", "--frame", "2048", "--hop", "512"], "1024-point frames expected")):
        with pytest.raises(SystemExit) as e:
            offline.main(bad + ["--out-dir", out])
        assert text in str(e.value), (bad, str(e.value))
