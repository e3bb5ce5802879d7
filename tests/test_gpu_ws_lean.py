"""vp_k_pitch_ws_l, the lean build of the single-block FAST wave-specialised pitch kernel (csrc/vp_pitch_ws_body.inc, WS_LEAN):

* bit-identity with the generic build (vp_set_wave_specialised(h, 2)) and with the phase kernel (h, 0): output, tracker state,
  undefined-behaviour counters and certified / fallback frame counts;
* the host launches it exactly where its constants hold, and a generic build everywhere else;
* a wait that runs out is still VP_ERR_TIMEOUT and a poisoned handle (the handled error path: the kernel runs to its end).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FS = 44100.0
VP_ERR_TIMEOUT = -9
LEAN = "vp_k_pitch_ws_l"
F, C = 1024, 256                      # the plugin's pitch frame and chunk at 44.1 kHz
BLOCKS = 13


def _x(S, T):
    """S streams of synth.make_streams, the LAST one all zeros (its gate stays closed)."""
    from vocoderproject_amd.synth import make_streams
    x = np.ascontiguousarray(make_streams(S, T).numpy())
    x[S - 1] = 0.0
    return x


def _entry_chunks(N, n_blocks):
    """nChunk at each block's entry -- bench.start_mix's rule: a chunk step starts a frame when nChunk is 0 or cpf - 1 (then it counts
    from 0 again), every step adds one; a block runs the steps whose start lies below N."""
    cpf = F // C
    pS, nCh, out = 0, 0, []
    for _ in range(n_blocks):
        out.append(nCh)
        while pS < N:
            if nCh == 0 or nCh == cpf - 1:
                nCh = 0
            nCh += 1
            pS += C
        pS -= N
    return out


def _state(p, s):
    d = p.pitch_state(s)
    d["a"] = d["a"].tobytes()
    return sorted(d.items())


def _run(x, N, ws, mono=False, iir="fast", yin="xcorr", n_blocks=BLOCKS, **params):
    """n_blocks blocks from a fresh prepare -> (output, states, ub counters, (certified, fallback), symbols launched)."""
    from vocoderproject_amd import BatchVocoderProcessor
    S = x.shape[0]
    params.setdefault("vocBool", 0)
    p = BatchVocoderProcessor(**params)
    p.prepareToPlay(FS, N, S)
    p.set_iir_mode(iir)
    p.set_yin_mode(yin)
    p.set_wave_specialised(ws)
    p.yin_certified_counts(reset=True)
    out, syms = np.empty((S, 2, N * n_blocks), np.float32), set()
    for b in range(n_blocks):
        blk = np.ascontiguousarray(x[:, :, b * N:(b + 1) * N])
        out[:, :, b * N:(b + 1) * N] = p.process_mono(np.ascontiguousarray(blk[:, 0])) if mono else p.process(blk)
        syms.add(p.debug_pitch_symbol())
    res = (out, [_state(p, s) for s in range(S)], p.ub_counters(), p.yin_certified_counts(reset=False), syms)
    p.close()
    return res


def _same(a, b, what):
    bad = np.argwhere(a[0] != b[0])
    assert bad.size == 0, f"{what}: {len(bad)} samples differ, first at {bad[0]}"
    assert a[0].tobytes() == b[0].tobytes(), f"{what}: output bits (signed zeros)"
    assert a[1] == b[1], f"{what}: pitch_state"
    assert a[2] == b[2], f"{what}: ub_counters {a[2]} {b[2]}"
    assert a[3] == b[3], f"{what}: yin_certified_counts {a[3]} {b[3]}"


@pytest.mark.parametrize("mono", [True, False], ids=["mono", "three-channel"])
@pytest.mark.parametrize("N", [256, 512, 1024])
def test_lean_build_is_bit_identical_to_the_generic_and_phase_kernels(N, mono):
    x = _x(3, N * BLOCKS)
    if mono:
        x[:, 1:] = 0.0
    assert {1, 2, 3} <= set(_entry_chunks(N, BLOCKS)), "all three block types"
    lean = _run(x, N, 1, mono)
    assert lean[4] == {LEAN}, lean[4]
    generic = _run(x, N, 2, mono)
    assert generic[4] == {"vp_k_pitch_ws"}, generic[4]
    phase = _run(x, N, 0, mono)
    assert not any(s.startswith("vp_k_pitch_ws") for s in phase[4]), phase[4]
    cert, fb = lean[3]
    assert cert > 0 and fb > 0, (cert, fb)                      # start-up frames take the fallback, settled ones the certified form
    assert np.abs(lean[0][:2]).max() > 0.01 and not lean[0][2].any()
    _same(lean, generic, "lean vs generic wave-specialised")
    _same(lean, phase, "lean vs phase kernel")


@pytest.mark.parametrize("name, kw", [
    ("N=1000", dict(N=1000)),
    ("exact", dict(iir="exact")),
    ("lpcPitch=14", dict(lpcPitch=14)),
    ("yin=direct", dict(yin="direct")),
    ("yin=force_fallback", dict(yin="xcorr_force_fallback")),
    ("vocoder on", dict(vocBool=1)),
    ("generic only", dict(ws=2)),
], ids=lambda v: v if isinstance(v, str) else "")
def test_everything_else_keeps_a_generic_build(name, kw):
    kw = dict(kw)
    N, ws = kw.pop("N", 1024), kw.pop("ws", 1)
    x = _x(2, N * 6)
    got = _run(x, N, ws, n_blocks=6, **kw)
    assert LEAN not in got[4] and all(got[4]), got[4]
    ref = _run(x, N, 0, n_blocks=6, **kw)
    assert not any(s.startswith("vp_k_pitch_ws") for s in ref[4]), ref[4]
    bad = np.argwhere(got[0] != ref[0])
    assert bad.size == 0, f"{name}: {len(bad)} samples differ from the phase kernel's, first at {bad[0]}"


@pytest.mark.parametrize("ws, sym", [(1, LEAN), (2, "vp_k_pitch_ws")], ids=["lean", "generic"])
def test_forced_wait_timeout_is_an_error_and_poisons_the_handle(ws, sym):
    """As tests/test_gpu_round6.py cuts them: ONE poll per wait.  The lean build marks the lost wait in LDS and raises the fault word
    once, at the launch's end: the host-visible behaviour is the generic build's (mode 2: that test's FAST case now runs the lean one)."""
    from vocoderproject_amd import BatchVocoderProcessor, VpError
    N, S = 1024, 6
    x = _x(S, N * 8)
    p = BatchVocoderProcessor(vocBool=0)
    p.prepareToPlay(FS, N, S)
    p.set_iir_mode("fast")
    p.set_yin_mode("xcorr")
    p.set_wave_specialised(ws)
    assert p.debug_pitch_symbol() == ""                      # (nothing launched since prepare)
    p.debug_set_spin_limit(1)
    codes = []
    for b in range(6):                                       # (the first frames of a run need no waits that can lose: keep going)
        try:
            p.process(np.ascontiguousarray(x[:, :, b * N:(b + 1) * N]))
            codes.append(0)
        except VpError as e:
            codes.append(e.code)
            assert "wait" in str(e) or "timed out" in str(e), str(e)
    assert p.debug_pitch_symbol() == sym                     # (a poisoned handle launches nothing more: the symbol stays)
    assert VP_ERR_TIMEOUT in codes, codes
    first = codes.index(VP_ERR_TIMEOUT)
    assert all(c == VP_ERR_TIMEOUT for c in codes[first:]), codes           # poisoned: every later call reports it
    with pytest.raises(VpError) as ei:
        p.synchronize()
    assert ei.value.code == VP_ERR_TIMEOUT
    assert round(p.debug_stamps(reset=False)[61] * 100.0) > 0               # (the debug counter agrees)
    p.debug_set_spin_limit(1 << 22)
    p.prepareToPlay(FS, N, S)                                               # prepare again: a clean handle, the same build, the same bits
    assert p.debug_pitch_symbol() == ""
    p.set_iir_mode("fast")
    p.set_yin_mode("xcorr")
    p.set_wave_specialised(ws)
    got = p.run(x[:, :, :N * 4])
    assert p.debug_pitch_symbol() == sym
    p.close()
    ref = _run(x[:, :, :N * 4], N, 0, n_blocks=4)
    assert got.tobytes() == ref[0].tobytes()
