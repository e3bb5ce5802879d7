"""The streaming pitch tracker and the streaming automatic correction on the GPU (include/vp_amd.h vp_pv_tracker_*,
vp_pv_autotune_blocks_device; kernels vp_k_yin_track_stream and vp_k_track_follow of csrc/vp_track.hip): period and followed ratio bit-equal
to tests/pv_track_stream_reference.py on every case of tests/pv_track_stream_cases.py (whose conditioning
tests/test_pv_track_stream_reference_cpu.py gates) however the blocks are grouped into calls, the raw decision against the batch kernel on
the same GPU, resets, the follow parameters and state across calls, autotune against its two parts, nullable outputs and keys, the
handle's allocations, batch independence, the neighbours on the shifter's handle, and argument errors."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: the process then has one HIP runtime, torch's)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pv_track_cases as TC  # noqa: E402
import pv_track_stream_cases as SC  # noqa: E402
import pv_track_stream_reference as SR  # noqa: E402

pytestmark = pytest.mark.gpu

PERIOD_SENTINEL = -777
VP_ERR_INVALID_ARG, VP_ERR_GEOMETRY = -1, -4


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(p, r, want_p, want_r):
    """Periods equal and ratios bit-equal; the first difference is what the assertion shows."""
    assert p.shape == want_p.shape and r.shape == want_r.shape
    bad = np.argwhere(p != want_p)
    assert bad.size == 0, ("period", len(bad), bad[:4].tolist(), p[tuple(bad[0])], want_p[tuple(bad[0])])
    bad = np.argwhere(_bits(r) != _bits(want_r))
    assert bad.size == 0, ("ratio", len(bad), bad[:4].tolist(), r[tuple(bad[0])], want_r[tuple(bad[0])])


def _call(trk, d_blocks, d_key=None, period=True, ratio=True):
    """vp_pv_tracker_process_blocks_device through the C ABI with sentinel-filled outputs: -> (rc, period or None, ratio or None), device tensors."""
    n = d_blocks.shape[0]
    d_p = torch.full((n, trk.S), PERIOD_SENTINEL, dtype=torch.int32, device="cuda") if period else None
    d_r = torch.full((n, trk.S), float("nan"), dtype=torch.float64, device="cuda") if ratio else None
    rc = trk.L.vp_pv_tracker_process_blocks_device(trk.h, d_blocks.data_ptr(), d_key.data_ptr() if d_key is not None else None,
                                                   d_p.data_ptr() if period else None, d_r.data_ptr() if ratio else None, n,
                                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return rc, d_p, d_r


def _feed(trk, d_in, groups, d_key=None, first=0):
    """The blocks d_in[first:first + sum(groups)] in calls of `groups` blocks -> (period, ratio) as NumPy arrays, every slot written."""
    ps, rs, b = [], [], first
    for k in groups:
        rc, d_p, d_r = _call(trk, d_in[b:b + k], d_key)
        assert rc == 0
        ps.append(d_p)
        rs.append(d_r)
        b += k
    torch.cuda.synchronize()
    p, r = torch.cat(ps).cpu().numpy(), torch.cat(rs).cpu().numpy()
    assert not np.any(p == PERIOD_SENTINEL) and not np.any(np.isnan(r))
    return p, r


def _tracker(c, S=None):
    from vocoderproject_amd import StreamingPitchTracker
    return StreamingPitchTracker(S or len(c.signals), c.N, c.fs, c.F, hold_blocks=c.hold, glide=c.glide)


# ---- 1. bit equality with the definition, however the blocks are grouped -------------------------------------------------------------------
@pytest.mark.parametrize("c", SC.CASES, ids=SC.case_id)
def test_period_and_ratio_equal_the_reference_in_every_grouping(c):
    ref_p, ref_r = SC.reference(c)
    d_in, d_key = _dev(SC.case_input(c), np.float32), _dev(c.keys, np.int32)
    for name, groups in SC.groupings(c).items():
        trk = _tracker(c)
        p, r = _feed(trk, d_in, groups, d_key)
        trk.close()
        try:
            _same(p, r, ref_p, ref_r)
        except AssertionError as e:
            raise AssertionError(f"{c.name} grouping {name} {groups}: {e}") from None


@pytest.mark.parametrize("c", [SC.BY_NAME[n] for n in ("n64", "n1000", "n4096")], ids=SC.case_id)
def test_raw_decision_equals_the_batch_kernel_on_the_window(c):
    """H = 0, g = 1: block b's ratio (n_b >= W) is vp_stft_track_pitch's for the row x[n_b - W, n_b) on the same GPU."""
    from vocoderproject_amd import StftRoundTrip, StreamingPitchTracker
    x = SC.case_input(c)
    S, W = len(c.signals), SC.window(c)
    trk = StreamingPitchTracker(S, c.N, c.fs, c.F)
    p, r = _feed(trk, _dev(x, np.float32), [c.n_blocks], _dev(c.keys, np.int32))
    trk.close()
    rows, fd = SC.rows(x), SC.first_decision(c)
    assert np.all(p[:fd] == 0) and np.all(r[:fd] == 1.0)
    # the windows of all decisions as the rows of one batch: row (b - fd) S + s, keys repeated
    wins = np.concatenate([rows[:, (b + 1) * c.N - W:(b + 1) * c.N] for b in range(fd, c.n_blocks)])
    st = StftRoundTrip(wins.shape[0], W, c.F, c.F // 2)                            # (rows of W samples: frame 0 reads the whole row)
    bp, br = st.track_pitch(_dev(wins, np.float32), c.fs, keys=list(c.keys) * (c.n_blocks - fd))
    torch.cuda.synchronize()
    st.close()
    _same(p[fd:], r[fd:], bp.cpu().numpy()[:, 0].reshape(-1, S), br.cpu().numpy()[:, 0].reshape(-1, S))
    assert np.any(p[fd:] > 0)


# ---- 2. resets and the follow state ---------------------------------------------------------------------------------------------------------
def test_reset_of_one_stream_and_of_all():
    c = SC.BY_NAME["n256-glide"]
    x, S, cut = SC.case_input(c), len(c.signals), 17
    d_in, d_key = _dev(x, np.float32), _dev(c.keys, np.int32)
    whole_p, whole_r = SC.reference(c)
    fresh_p, fresh_r = SR.run(x[cut:], c.fs, c.F, c.keys, c.hold, c.glide)
    trk = _tracker(c)
    _feed(trk, d_in, [5, 12], d_key)
    trk.reset(2)
    p, r = _feed(trk, d_in, [3, 1, c.n_blocks - cut - 4], d_key, first=cut)
    want_p, want_r = whole_p[cut:].copy(), whole_r[cut:].copy()
    want_p[:, 2], want_r[:, 2] = fresh_p[:, 2], fresh_r[:, 2]                       # that stream is a fresh handle's; the others carry on
    _same(p, r, want_p, want_r)
    trk.reset()                                                                    # every stream, issued twice and once more per stream:
    trk.reset(-1)                                                                  # pending resets do not add up
    for s in range(S):
        trk.reset(s)
    p, r = _feed(trk, d_in, [c.n_blocks - cut], d_key, first=cut)
    _same(p, r, fresh_p, fresh_r)
    trk.close()


def test_reset_of_more_streams_than_one_update_launch_carries():
    """40 streams, 21 of them reset: the resets travel in two launches in front of the call."""
    from vocoderproject_amd import StreamingPitchTracker
    c = SC.BY_NAME["n1024-44k"]
    S, cut = 40, 4
    names = [c.signals[s % len(c.signals)] for s in range(S)]
    keys = [c.keys[s % len(c.keys)] for s in range(S)]
    x = TC.make_input(names, c.n_blocks * c.N, c.fs, 9)
    x = np.ascontiguousarray(x.reshape(S, c.n_blocks, c.N).transpose(1, 0, 2))
    whole_p, whole_r = SR.run(x, c.fs, c.F, keys, 2, 0.5)
    fresh_p, fresh_r = SR.run(x[cut:], c.fs, c.F, keys, 2, 0.5)
    trk = StreamingPitchTracker(S, c.N, c.fs, c.F, hold_blocks=2, glide=0.5)
    d_in, d_key = _dev(x, np.float32), _dev(keys, np.int32)
    _feed(trk, d_in, [cut], d_key)
    hit = list(range(0, S, 2)) + [S - 1]
    for s in hit:
        trk.reset(s)
    p, r = _feed(trk, d_in, [2, c.n_blocks - cut - 2], d_key, first=cut)
    trk.close()
    want_p, want_r = whole_p[cut:].copy(), whole_r[cut:].copy()
    want_p[:, hit], want_r[:, hit] = fresh_p[:, hit], fresh_r[:, hit]
    assert not np.array_equal(want_p, whole_p[cut:])
    _same(p, r, want_p, want_r)


def test_set_follow_takes_effect_at_the_next_call_and_the_state_carries():
    """The hold of the N = 256 cases spans call boundaries (the gap lasts twelve blocks, the calls are shorter), the glide is changed
    mid-way: the tables are the reference's with the same changes between the same blocks."""
    c = SC.BY_NAME["n256-hold3"]
    x, S = SC.case_input(c), len(c.signals)
    d_in, d_key = _dev(x, np.float32), _dev(c.keys, np.int32)
    plan = [(15, 3, 1.0), (4, 3, 1.0), (6, 1000, 0.5), (7, 0, 1.0), (8, 2, 0.25)]   # (blocks, hold, glide): the gap starts at block 17
    assert sum(k for k, _, _ in plan) == c.n_blocks
    ref = SR.StreamTracker(S, c.N, c.fs, c.F)
    trk = _tracker(c)
    b = 0
    for k, hold, glide in plan:
        ref.set_follow(hold, glide)
        want_p, want_r = ref.process(x[b:b + k], c.keys)
        trk.set_follow(hold, glide)
        rc, d_p, d_r = _call(trk, d_in[b:b + k], d_key)
        trk.set_follow(7, 0.125)                                                   # after the call was issued: it does not see this
        torch.cuda.synchronize()
        assert rc == 0
        _same(d_p.cpu().numpy(), d_r.cpu().numpy(), want_p, want_r)
        b += k
    trk.close()


# ---- 3. autotune against its parts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,hop", [("n256-glide", 256), ("n64", 128), ("n1000", 256)])
def test_autotune_is_the_tracker_then_the_curve_call(name, hop):
    from vocoderproject_amd import PhaseVocoderStream
    c = SC.BY_NAME[name]
    S = len(c.signals)
    d_in, d_key = _dev(SC.case_input(c), np.float32), _dev(c.keys, np.int32)
    groups = SC.groupings(c)["mixed"]
    # the parts: the tracker call, then the curve call along its table
    trk, pv = _tracker(c), PhaseVocoderStream(S, c.N, hop)
    d_parts = torch.full_like(d_in, float("nan"))
    ps, rs, b = [], [], 0
    for k in groups:
        rc, d_p, d_r = _call(trk, d_in[b:b + k], d_key)
        assert rc == 0
        pv.process_device(d_in[b:b + k], d_parts[b:b + k], n_blocks=k, d_ratio=d_r)
        ps.append(d_p)
        rs.append(d_r)
        b += k
    torch.cuda.synchronize()
    trk.close()
    pv.close()
    p, r = torch.cat(ps).cpu().numpy(), torch.cat(rs).cpu().numpy()
    _same(p, r, *SC.reference(c))
    # the one call, through the C ABI (with and without a period table) and through Python
    outs = []
    for variant in ("c", "c-no-period", "python"):
        trk, pv = _tracker(c), PhaseVocoderStream(S, c.N, hop)
        d_out = torch.full_like(d_in, float("nan"))
        ps, rs, b = [], [], 0
        for k in groups:
            if variant == "python":
                d_p, d_r = pv.autotune_device(trk, d_in[b:b + k], d_out[b:b + k], n_blocks=k, keys=list(c.keys))
            else:
                d_p = torch.full((k, S), PERIOD_SENTINEL, dtype=torch.int32, device="cuda")
                d_r = torch.full((k, S), float("nan"), dtype=torch.float64, device="cuda")
                rc = pv.L.vp_pv_autotune_blocks_device(pv.h, trk.h, d_in[b:b + k].data_ptr(), d_out[b:b + k].data_ptr(), d_key.data_ptr(),
                                                       d_p.data_ptr() if variant == "c" else None, d_r.data_ptr(), k,
                                                       C.c_void_p(torch.cuda.current_stream().cuda_stream))
                assert rc == 0
            ps.append(d_p)
            rs.append(d_r)
            b += k
        torch.cuda.synchronize()
        trk.close()
        pv.close()
        if variant != "c-no-period":
            _same(torch.cat(ps).cpu().numpy(), torch.cat(rs).cpu().numpy(), p, r)
        else:
            assert np.array_equal(_bits(torch.cat(rs).cpu().numpy()), _bits(r))
        outs.append(d_out.cpu().numpy())
    y = d_parts.cpu().numpy()
    assert np.all(np.isfinite(y)) and np.abs(y).max() > 0.1
    for o in outs:
        assert np.array_equal(o.view(np.uint32), y.view(np.uint32))


def test_autotune_of_an_unvoiced_batch_is_the_zero_shift():
    from vocoderproject_amd import PhaseVocoderStream, StreamingPitchTracker
    fs, N, nb = 44100.0, 256, 12
    x = TC.make_input(("noise", "silence", "noise", "noise"), nb * N, fs, 5)
    x[2] = x[2, ::-1] * np.float32(0.01)
    x[3] *= np.float32(0.1)
    d_in = _dev(x.reshape(4, nb, N).transpose(1, 0, 2), np.float32)
    trk, pv, pv0 = StreamingPitchTracker(4, N, fs, hold_blocks=2, glide=0.5), PhaseVocoderStream(4, N), PhaseVocoderStream(4, N)
    d_out, d_zero = torch.full_like(d_in, float("nan")), torch.full_like(d_in, float("nan"))
    p, r = pv.autotune_device(trk, d_in, d_out, n_blocks=nb)
    pv0.process_device(d_in, d_zero, n_blocks=nb)
    torch.cuda.synchronize()
    for h in (trk, pv, pv0):
        h.close()
    assert np.all(p.cpu().numpy() == 0) and np.all(r.cpu().numpy() == 1.0)
    assert np.array_equal(d_out.cpu().numpy().view(np.uint32), d_zero.cpu().numpy().view(np.uint32))


def test_run_with_a_tracker_streams_whole_signals():
    from vocoderproject_amd import PhaseVocoderStream, StreamingPitchTracker
    x, keys = TC.steady_input()
    S, T = x.shape
    N = 256
    trk, pv = StreamingPitchTracker(S, N, TC.STEADY_FS), PhaseVocoderStream(S, N)
    y, p, r = pv.run(x, blocks_per_call=5, autotune=trk, keys=keys)
    nb = -(-(T + pv.latency) // N)
    trk.close()
    pv.close()
    assert y.shape == x.shape and p.shape == r.shape == (nb, S)
    xp = np.zeros((S, nb * N), np.float32)
    xp[:, :T] = x
    want_p, want_r = SR.run(np.ascontiguousarray(xp.reshape(S, nb, N).transpose(1, 0, 2)), TC.STEADY_FS, 1024, keys)
    _same(p, r, want_p, want_r)
    assert np.all(np.isfinite(y)) and np.abs(y).max() > 0.1


# ---- 4. nullable outputs and keys -------------------------------------------------------------------------------------------------------------
def test_nullable_outputs_and_keys():
    """A call without one of its tables advances the state like any other (the handle's scratch stands in, 64 blocks per launch pair: the 70
    blocks here take two), so the calls after it give the same bits."""
    c = SC.BY_NAME["n64"]
    S = len(c.signals)
    x = np.concatenate([SC.case_input(c), SC.case_input(c)[:30]])                   # 70 blocks
    d_in, d_key = _dev(x, np.float32), _dev(c.keys, np.int32)
    want_p, want_r = SR.run(x, c.fs, c.F, c.keys, 2, 0.5)
    for period, ratio in ((True, True), (True, False), (False, True)):
        trk = _tracker(c)
        trk.set_follow(2, 0.5)
        rc, d_p, d_r = _call(trk, d_in[:66], d_key, period=period, ratio=ratio)
        assert rc == 0
        p2, r2 = _feed(trk, d_in, [4], d_key, first=66)
        trk.close()
        if period:
            assert np.array_equal(d_p.cpu().numpy(), want_p[:66])
        if ratio:
            assert np.array_equal(_bits(d_r.cpu().numpy()), _bits(want_r[:66]))
        _same(p2, r2, want_p[66:], want_r[66:])
    # NULL = chromatic = what -1 and 13 count as; another key changes the ratio
    base = None
    for keys in (None, (12,) * S, (-1, 13, 12, -5, 99, 12), (0,) * S):
        trk = _tracker(c)
        p, r = _feed(trk, d_in, [40], None if keys is None else _dev(keys, np.int32))
        trk.close()
        if base is None:
            base = (p, r)
        elif keys == (0,) * S:
            assert np.array_equal(p, base[0]) and not np.array_equal(_bits(r), _bits(base[1]))
        else:
            _same(p, r, *base)


# ---- 5. the handle and its neighbours -----------------------------------------------------------------------------------------------------------
def test_allocations_are_made_at_create_only():
    c = SC.BY_NAME["n1024-44k"]
    trk = _tracker(c)
    n0 = trk.debug_alloc_count()
    assert n0 > 0
    d_in = _dev(SC.case_input(c), np.float32)
    _feed(trk, d_in, [1, 3, 5])
    trk.reset(1)
    trk.set_follow(5, 0.5)
    rc, _, _ = _call(trk, d_in, period=False)
    torch.cuda.synchronize()
    assert rc == 0 and trk.debug_alloc_count() == n0
    trk.close()


def test_streams_do_not_see_their_neighbours():
    from vocoderproject_amd import StreamingPitchTracker
    fs, F, N, nb = 44100.0, 1024, 256, 14
    voiced = TC.make_input(("sine_off", "glide", "gap"), nb * N, fs, 11)
    noise = TC.make_input(("noise",), nb * N, fs, 12)[0]
    silent = np.zeros(nb * N, np.float32)
    keys = (0, 7, 12)

    def run(rows, ks):
        trk = StreamingPitchTracker(len(rows), N, fs, F, hold_blocks=1, glide=0.5)
        d_in = _dev(np.stack(rows).reshape(len(rows), nb, N).transpose(1, 0, 2), np.float32)
        out = _feed(trk, d_in, [3, nb - 3], _dev(ks, np.int32))
        trk.close()
        return out

    p_a, r_a = run([voiced[0], noise, voiced[1], silent, voiced[2]], (keys[0], 12, keys[1], 12, keys[2]))
    p_b, r_b = run([voiced[0], silent, voiced[1], noise, voiced[2]] + [noise] * 14, (keys[0], 12, keys[1], 12, keys[2]) + (3,) * 14)   # 19 streams: two follow groups
    p_c, r_c = run([voiced[0], voiced[1], voiced[2]], keys)
    assert np.any(p_c > 0)
    for i, j in enumerate((0, 2, 4)):
        _same(p_a[:, j], r_a[:, j], p_c[:, i], r_c[:, i])
        _same(p_b[:, j], r_b[:, j], p_c[:, i], r_c[:, i])
    assert np.all(p_a[:, 3] == 0) and np.all(p_b[:, 1] == 0) and np.array_equal(p_a[:, 1], p_b[:, 3])


def test_plain_and_curve_calls_on_the_shifter_are_unaffected_between_autotune_calls():
    from vocoderproject_amd import PhaseVocoderStream, semitones_to_ratios
    c = SC.BY_NAME["n256-glide"]
    S = len(c.signals)
    d_in = _dev(SC.case_input(c), np.float32)
    curve = _dev(np.repeat(semitones_to_ratios(np.linspace(-4.0, 4.0, S))[None, :], 8, axis=0), np.float64)

    def sequence(with_tracker):
        """blocks 0..7 plain at +3, 8..15 autotune (or the curve call along the reference's table), 16..23 curve, 24..31 plain."""
        pv, trk = PhaseVocoderStream(S, c.N), _tracker(c)
        pv.set_semitones(3.0)
        d_out = torch.full_like(d_in[:32], float("nan"))
        pv.process_device(d_in[0:8], d_out[0:8], n_blocks=8)
        if with_tracker:
            _feed(trk, d_in, [8], _dev(c.keys, np.int32))                          # (the tracker has heard blocks 0..7 too, in its keys)
            pv.autotune_device(trk, d_in[8:16], d_out[8:16], n_blocks=8, keys=list(c.keys))
        else:
            pv.process_device(d_in[8:16], d_out[8:16], n_blocks=8, d_ratio=_dev(SC.reference(c)[1][8:16], np.float64))
        pv.process_device(d_in[16:24], d_out[16:24], n_blocks=8, d_ratio=curve)
        pv.process_device(d_in[24:32], d_out[24:32], n_blocks=8)
        torch.cuda.synchronize()
        pv.close()
        trk.close()
        return d_out.cpu().numpy()

    a, b = sequence(True), sequence(False)
    assert np.all(np.isfinite(a)) and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 6. argument errors ---------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_are_statuses_and_launch_nothing():
    from vocoderproject_amd import PhaseVocoderStream, StreamingPitchTracker, VpError
    for kw in (dict(sample_rate=7999.0), dict(sample_rate=51201.0), dict(frame_len=512), dict(frame_len=4096), dict(n_streams=0), dict(block_size=0)):
        a = dict(n_streams=2, block_size=256, sample_rate=44100.0, frame_len=1024)
        a.update(kw)
        with pytest.raises(VpError) as e:
            StreamingPitchTracker(**a)
        assert e.value.code == (VP_ERR_GEOMETRY if "frame_len" in kw else VP_ERR_INVALID_ARG)
    trk = StreamingPitchTracker(2, 256, 44100.0)
    for hold, glide in ((-1, 1.0), ((1 << 20) + 1, 1.0), (0, 0.0), (0, -0.5), (0, 1.0000001), (0, float("nan")), (0, float("inf"))):
        with pytest.raises(VpError) as e:
            trk.set_follow(hold, glide)
        assert e.value.code == VP_ERR_INVALID_ARG
    trk.set_follow(1 << 20, 1.0)
    trk.set_follow(0, 1.0)
    for s in (-2, 2):
        with pytest.raises(VpError):
            trk.reset(s)
    d_in = _dev(np.zeros((6, 2, 256)), np.float32)
    rc, d_p, d_r = _call(trk, d_in, period=False, ratio=False)
    assert rc == VP_ERR_INVALID_ARG
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    d_p = torch.full((6, 2), PERIOD_SENTINEL, dtype=torch.int32, device="cuda")
    d_r = torch.full((6, 2), float("nan"), dtype=torch.float64, device="cuda")
    d_out = torch.full_like(d_in, float("nan"))
    L = trk.L
    assert L.vp_pv_tracker_process_blocks_device(trk.h, None, None, d_p.data_ptr(), d_r.data_ptr(), 6, st) == VP_ERR_INVALID_ARG
    for n in (0, -3):
        assert L.vp_pv_tracker_process_blocks_device(trk.h, d_in.data_ptr(), None, d_p.data_ptr(), d_r.data_ptr(), n, st) == VP_ERR_INVALID_ARG
    pv = PhaseVocoderStream(2, 256)
    args = lambda p, t, o, r, n: L.vp_pv_autotune_blocks_device(p, t, d_in.data_ptr(), o, None, d_p.data_ptr(), r, n, st)   # noqa: E731
    assert args(None, trk.h, d_out.data_ptr(), d_r.data_ptr(), 6) == VP_ERR_INVALID_ARG
    assert args(pv.h, None, d_out.data_ptr(), d_r.data_ptr(), 6) == VP_ERR_INVALID_ARG
    assert args(pv.h, trk.h, None, d_r.data_ptr(), 6) == VP_ERR_INVALID_ARG
    assert args(pv.h, trk.h, d_out.data_ptr(), None, 6) == VP_ERR_INVALID_ARG          # the ratio table is required
    assert args(pv.h, trk.h, d_out.data_ptr(), d_r.data_ptr(), 0) == VP_ERR_INVALID_ARG
    for S, N in ((3, 256), (2, 128)):                                                  # mismatched handles
        other = PhaseVocoderStream(S, N)
        assert args(other.h, trk.h, d_out.data_ptr(), d_r.data_ptr(), 1) == VP_ERR_GEOMETRY
        other.close()
    torch.cuda.synchronize()
    assert np.all(d_p.cpu().numpy() == PERIOD_SENTINEL) and np.all(np.isnan(d_r.cpu().numpy())) and np.all(np.isnan(d_out.cpu().numpy()))   # nothing ran
    rc, d_p, d_r = _call(trk, d_in)                                                    # and the handle still serves a good call
    torch.cuda.synchronize()
    pv.close()
    trk.close()
    assert rc == 0 and np.all(d_p.cpu().numpy() == 0) and np.all(d_r.cpu().numpy() == 1.0)
