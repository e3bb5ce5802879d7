"""The streaming phase vocoder on the GPU (include/vp_amd.h vp_pv_*, csrc/vp_stft.hip vp_k_pv_stream): bit-identical to the one-shot
vp_stft_pitch_shift delayed by the latency, whatever the call grouping; interval changes and resets ordered with the calls;
no allocation in process calls; coexistence with the other handles."""
import math
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: the process then has one HIP runtime, torch's)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

INTERVALS = [-12, -5, 0, 3, 7, 12, -7, 5]


def _signals(S, T, seed=0, fs=48000.0):
    """Harmonic tones with a little noise, a different pitch per stream."""
    rng = np.random.default_rng(seed)
    t = np.arange(T) / fs
    x = np.zeros((S, T))
    for s in range(S):
        f0 = 110.0 * 2 ** (s % 24 / 12)
        for h in range(1, 6):
            x[s] += 0.3 / h * np.sin(2 * np.pi * f0 * h * t + rng.uniform(0, 2 * np.pi))
        x[s] += 0.01 * rng.standard_normal(T)
    return x.astype(np.float32)


def _stream(ps, x, calls):
    """x [S][T] (T = whole blocks) through ps.process_device in calls of calls[i % len] blocks (no synchronisation between calls)."""
    import torch
    S, T = x.shape
    N = ps.N
    nb = T // N
    d_in = torch.from_numpy(np.ascontiguousarray(x.reshape(S, nb, N).transpose(1, 0, 2))).cuda()
    d_out = torch.full_like(d_in, float("nan"))
    b, i = 0, 0
    while b < nb:
        k = min(calls[i % len(calls)], nb - b)
        ps.process_device(d_in[b:b + k], d_out[b:b + k], n_blocks=k)
        b += k
        i += 1
    torch.cuda.synchronize()
    return d_out.cpu().numpy().transpose(1, 0, 2).reshape(S, T)


def _one_shot(x, semis, hop):
    """vp_stft_pitch_shift per stream with its own interval (one batch call per distinct interval)."""
    import torch
    from vocoderproject_amd import StftRoundTrip
    S, T = x.shape
    st = StftRoundTrip(S, T, 1024, hop)
    d_in = torch.from_numpy(x).cuda()
    d_out = torch.zeros_like(d_in)
    y = np.zeros_like(x)
    for v in sorted(set(semis)):
        st.pitch_shift(d_in, d_out, float(v))
        torch.cuda.synchronize()
        o = d_out.cpu().numpy()
        for s in range(S):
            if semis[s] == v:
                y[s] = o[s]
    st.close()
    return y


def _assert_one_shot(y, ref, L, what):
    T = y.shape[1]
    assert np.all(y[:, :L] == 0), what
    for s in range(y.shape[0]):
        if not np.array_equal(y[s, L:], ref[s, :T - L]):
            d = np.nonzero(y[s, L:] != ref[s, :T - L])[0]
            raise AssertionError(f"{what}: stream {s} differs at {d.size} samples from {d[0]}, max "
                                 f"{np.abs(y[s, L:] - ref[s, :T - L]).max():.3g}")


@pytest.mark.parametrize("N,hop,n_blocks", [(64, 256, 200), (100, 256, 130), (256, 256, 48), (1024, 256, 14), (4096, 256, 5),
                                            (256, 128, 48)])
def test_bit_identical_to_one_shot(N, hop, n_blocks):
    from vocoderproject_amd import PhaseVocoderStream
    S = 8
    x = _signals(S, N * n_blocks, seed=N)
    ps = PhaseVocoderStream(S, N, hop=hop)
    assert ps.latency == 1024 - math.gcd(N, hop)
    for s, v in enumerate(INTERVALS):
        ps.set_semitones(v, stream=s)
    y = _stream(ps, x, [1, 3, 16])
    _assert_one_shot(y, _one_shot(x, INTERVALS, hop), ps.latency, f"N={N} hop={hop}")


def test_bit_identical_at_256_streams():
    from vocoderproject_amd import PhaseVocoderStream
    S, N = 256, 1024
    semis = [INTERVALS[s % len(INTERVALS)] for s in range(S)]
    x = _signals(S, N * 24, seed=7)
    ps = PhaseVocoderStream(S, N)
    for s, v in enumerate(semis):
        ps.set_semitones(v, stream=s)
    y = _stream(ps, x, [1, 3, 16])
    _assert_one_shot(y, _one_shot(x, semis, 256), ps.latency, "S=256")


def test_run_aligns_output_with_input():
    from vocoderproject_amd import PhaseVocoderStream
    S, N = 4, 100
    x = _signals(S, 5000, seed=3)
    ps = PhaseVocoderStream(S, N)
    ps.set_semitones(4)
    y = ps.run(x, blocks_per_call=5)
    L = ps.latency
    T = -(-(5000 + L) // N) * N
    xp = np.zeros((S, T), np.float32)
    xp[:, :5000] = x
    ref = _one_shot(xp, [4] * S, 256)
    assert y.shape == x.shape and np.array_equal(y, ref[:, :5000])


def test_call_grouping_does_not_change_a_bit():
    from vocoderproject_amd import PhaseVocoderStream
    S, N, nb = 4, 256, 48
    x = _signals(S, N * nb, seed=11)
    outs = []
    for mode in ("host", "dev1", "dev16"):
        ps = PhaseVocoderStream(S, N)
        ps.set_semitones(-3)
        ps.set_semitones(9, stream=2)
        if mode == "host":
            outs.append(np.concatenate([ps.process(x[:, b * N:(b + 1) * N]) for b in range(nb)], axis=1))
        else:
            outs.append(_stream(ps, x, [1] if mode == "dev1" else [16]))
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])


def _schedule_run(x, N, calls, changes, device=True):
    """Streams x [S][T]; changes: {call index: [(stream, semitones), ...]} applied before that call.  Returns the output and, per
    stream, the ratio of every call (the restatement's schedule)."""
    import torch
    from vocoderproject_amd import PhaseVocoderStream
    S, T = x.shape
    ps = PhaseVocoderStream(S, N)
    ps.set_semitones(2)
    nb = T // N
    d_in = torch.from_numpy(np.ascontiguousarray(x.reshape(S, nb, N).transpose(1, 0, 2))).cuda()
    d_out = torch.zeros_like(d_in)
    b, i, spans = 0, 0, []
    semi = [2.0] * S
    while b < nb:
        for s, v in changes.get(i, []):
            ps.set_semitones(v, stream=s)
            semi[s] = float(v)
        k = min(calls[i % len(calls)], nb - b)
        ps.process_device(d_in[b:b + k], d_out[b:b + k], n_blocks=k)
        spans.append((k, list(semi)))
        b += k
        i += 1
    torch.cuda.synchronize()
    return d_out.cpu().numpy().transpose(1, 0, 2).reshape(S, T), spans


def _restated(x, N, spans, shift=0):
    """The restatement with the interval schedule; shift = +-1 applies every change one call late / early."""
    import pv_stream_reference as P
    S = x.shape[0]
    y = np.zeros(x.shape)
    for s in range(S):
        r = P.PvStreamRef(N)
        pos, out = 0, []
        for i, (k, semi) in enumerate(spans):
            j = min(max(i - shift, 0), len(spans) - 1)
            out.append(r.process(x[s, pos:pos + k * N], 2.0 ** (spans[j][1][s] / 12.0)))
            pos += k * N
        y[s] = np.concatenate(out)
    return y


def test_interval_changes_follow_the_calls():
    S, N = 4, 256
    x = _signals(S, N * 40, seed=5).astype(np.float64).astype(np.float32)
    changes = {3: [(1, -7)], 6: [(3, 12), (1, 5)], 9: [(0, -12)], 12: [(3, -4)]}
    y, spans = _schedule_run(x, N, [1, 3, 2], changes)
    ref = _restated(x.astype(np.float64), N, spans)
    err = y - ref
    rms = np.sqrt(np.mean(err ** 2))
    frac = np.mean(np.abs(err) > 1e-5)
    assert rms < 1e-4 and frac < 1e-3, (rms, frac)
    for sh in (-1, 1):                     # the test sees a change applied one call early or late
        bad = _restated(x.astype(np.float64), N, spans, shift=sh)
        e = y - bad
        assert np.sqrt(np.mean(e ** 2)) > 1e-4 or np.mean(np.abs(e) > 1e-5) > 1e-3, sh


def test_reset_of_one_stream():
    from vocoderproject_amd import PhaseVocoderStream
    S, N, nb, k0 = 4, 256, 40, 18
    x = _signals(S, N * nb, seed=9)
    calls = [3]                            # calls of three blocks; the reset goes in before the call that starts at block k0
    base = PhaseVocoderStream(S, N)
    base.set_semitones(5)
    y0 = _stream(base, x, calls)
    ps = PhaseVocoderStream(S, N)
    ps.set_semitones(5)
    ya = _stream(ps, x[:, :k0 * N], calls)
    ps.reset(2)
    yb = _stream(ps, x[:, k0 * N:], calls)
    y = np.concatenate([ya, yb], axis=1)
    for s in (0, 1, 3):
        assert np.array_equal(y[s], y0[s]), s
    fresh = PhaseVocoderStream(1, N)
    fresh.set_semitones(5)
    yf = _stream(fresh, np.ascontiguousarray(x[2:3, k0 * N:]), calls)
    assert np.array_equal(yb[2], yf[0])
    assert np.array_equal(ya[2], y0[2, :k0 * N])


def test_a_tone_moves_by_seven_semitones():
    from vocoderproject_amd import PhaseVocoderStream
    fs, N = 48000.0, 256
    T = N * 400
    x = (0.5 * np.sin(2 * np.pi * 440.0 * np.arange(T) / fs)).astype(np.float32)[None]
    ps = PhaseVocoderStream(1, N)
    ps.set_semitones(7)
    y = ps.run(x, blocks_per_call=16)[0, 4096:]
    spec = np.abs(np.fft.rfft(y * np.hanning(len(y))))
    f = np.fft.rfftfreq(len(y), 1 / fs)[np.argmax(spec)]
    assert abs(f - 440.0 * 2 ** (7 / 12)) < 3.0, f
    assert np.sqrt(np.mean(y ** 2)) > 0.1


def test_errors_and_no_allocation_in_process_calls():
    import torch
    from vocoderproject_amd import PhaseVocoderStream, VpError
    S, N = 3, 128
    ps = PhaseVocoderStream(S, N, hop=512)
    assert ps.latency == 1024 - 128
    for bad in (lambda: ps.set_semitones(12.5), lambda: ps.set_semitones(1, stream=3), lambda: ps.set_semitones(1, stream=-2),
                lambda: ps.reset(3), lambda: ps.semitones(-1), lambda: PhaseVocoderStream(2, 256, frame_len=2048),
                lambda: PhaseVocoderStream(2, 256, hop=300), lambda: PhaseVocoderStream(0, 256)):
        with pytest.raises(VpError):
            bad()
    assert ps.L.vp_pv_process_blocks_device(ps.h, 0, 0, 1, None) == -1
    d = torch.zeros(2, S, N, device="cuda")
    assert ps.L.vp_pv_process_blocks_device(ps.h, d.data_ptr(), d.data_ptr(), 0, None) == -1
    n0 = ps.debug_alloc_count()
    assert n0 > 0
    x = _signals(S, N * 40, seed=1)
    for i in range(40):
        if i % 7 == 0:
            ps.set_semitones(i % 12, stream=-1 if i % 2 else 1)
        if i % 11 == 0:
            ps.reset(i % S)
        ps.process(x[:, i * N:(i + 1) * N])
    # more pending changes than one call carries: the update launches in front of it
    for s in range(S):
        ps.set_semitones(-s, stream=s)
        ps.reset(s)
    _stream(ps, x, [1, 4])
    assert ps.debug_alloc_count() == n0
    assert ps.semitones(2) == -2.0


def test_many_pending_changes_match_few():
    """More than VP_PV_MAX_UPDATES pending changes go through update launches: same result as the same state set directly."""
    from vocoderproject_amd import PhaseVocoderStream
    S, N = 40, 256
    x = _signals(S, N * 12, seed=2)
    a = PhaseVocoderStream(S, N)
    b = PhaseVocoderStream(S, N)
    semis = [(s % 25) - 12 for s in range(S)]
    for s in range(S):
        a.set_semitones(semis[s], stream=s)
    ya = _stream(a, x, [4])
    b.set_semitones(0)
    _stream(b, x[:, :4 * N], [4])
    for s in range(S):
        b.set_semitones(semis[s], stream=s)
        b.reset(s)
    yb = _stream(b, x, [4])
    assert np.array_equal(ya, yb)


def test_handles_coexist():
    import torch
    from vocoderproject_amd import BatchVocoderProcessor, PhaseVocoderStream, StftRoundTrip
    S, N, T = 2, 256, 256 * 24
    x = _signals(S, T, seed=4)
    # alone first
    v_alone = BatchVocoderProcessor()
    v_alone.prepareToPlay(44100.0, 256, S)
    xin = np.zeros((S, 3, T), np.float32)
    xin[:, 0] = x
    y_v_alone = np.concatenate([v_alone.process(np.ascontiguousarray(xin[:, :, b * 256:(b + 1) * 256])) for b in range(T // 256)], axis=2)
    ref_pv = _one_shot(x, [7, 7], 256)
    # then side by side, launches interleaved
    v = BatchVocoderProcessor()
    v.prepareToPlay(44100.0, 256, S)
    ps = PhaseVocoderStream(S, N)
    ps.set_semitones(7)
    st = StftRoundTrip(S, T, 1024, 256)
    d_x = torch.from_numpy(x).cuda()
    d_rt = torch.zeros_like(d_x)
    ys_v, ys_pv = [], []
    for b in range(T // N):
        ys_v.append(v.process(np.ascontiguousarray(xin[:, :, b * 256:(b + 1) * 256])))
        ys_pv.append(ps.process(x[:, b * N:(b + 1) * N]))
        if b % 8 == 0:
            st(d_x, d_rt)
    torch.cuda.synchronize()
    assert np.array_equal(np.concatenate(ys_v, axis=2), y_v_alone)
    _assert_one_shot(np.concatenate(ys_pv, axis=1), ref_pv, ps.latency, "beside the other handles")
    rt = d_rt.cpu().numpy()
    assert np.abs(rt[:, 1024:T - 1024] - x[:, 1024:T - 1024]).max() < 1e-5
