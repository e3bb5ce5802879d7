"""The pitch trackers on the GPU at the edges of the walk, the note table and the ring (kernels vp_k_yin_track, vp_k_yin_track_stream and
vp_k_track_follow of csrc/vp_track.hip, shared body csrc/vp_track_body.inc): period equal and ratio bit-equal to the definition on every
case of tests/pv_track_edge_cases.py, whose branches tests/test_pv_track_edges_cpu.py asserts reached -- the popped slot behind the note
table, first == tau0, first at both sides of every ballot word, the walk's last lag from both sides, tauMax at every residue mod 8, exact
zeros and NaNs in the function, 299 streams with a partial last workgroup -- the streaming kernel at the block sizes whose gather carries
(N = 1, 24, 48, 63, 65, 100) in every grouping of the calls and against the batch kernel on the window, and the two autotune entry points
on top-of-range input against their parts.  All comparisons are exact (int32, and float64 by bits).

What this file sees that tests/test_gpu_pv_track.py and tests/test_gpu_pv_track_stream.py do not is recorded, fault by fault, in
profiles/pv_track_mutations.txt.  Runtime on an MI355X: 2.9 s for the file (88 tests), 2.5 s on the LDS-poisoning twin."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: the process then has one HIP runtime, torch's)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pv_track_edge_cases as EC  # noqa: E402
import pv_track_stream_cases as SC  # noqa: E402

pytestmark = pytest.mark.gpu

PERIOD_SENTINEL = -777


# ---- helpers (those of tests/test_gpu_pv_track.py and tests/test_gpu_pv_track_stream.py) -----------------------------------------------------
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


def _raw_track(st, d_in, fs, d_key):
    """vp_stft_track_pitch through the C ABI with sentinel-filled outputs -> (period, ratio) as NumPy arrays, every slot written."""
    d_p = torch.full((st.S, st.n_frames), PERIOD_SENTINEL, dtype=torch.int32, device="cuda")
    d_r = torch.full((st.S, st.n_frames), float("nan"), dtype=torch.float64, device="cuda")
    rc = st.L.vp_stft_track_pitch(st.h, d_in.data_ptr(), float(fs), d_key.data_ptr(), d_p.data_ptr(), d_r.data_ptr(),
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0
    p, r = d_p.cpu().numpy(), d_r.cpu().numpy()
    assert not np.any(p == PERIOD_SENTINEL) and not np.any(np.isnan(r))
    return p, r


def _call(trk, d_blocks, d_key):
    """vp_pv_tracker_process_blocks_device through the C ABI with sentinel-filled outputs -> (period, ratio), device tensors."""
    n = d_blocks.shape[0]
    d_p = torch.full((n, trk.S), PERIOD_SENTINEL, dtype=torch.int32, device="cuda")
    d_r = torch.full((n, trk.S), float("nan"), dtype=torch.float64, device="cuda")
    rc = trk.L.vp_pv_tracker_process_blocks_device(trk.h, d_blocks.data_ptr(), d_key.data_ptr(), d_p.data_ptr(), d_r.data_ptr(), n,
                                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    return d_p, d_r


def _feed(trk, d_in, groups, d_key):
    ps, rs, b = [], [], 0
    for k in groups:
        d_p, d_r = _call(trk, d_in[b:b + k], d_key)
        ps.append(d_p)
        rs.append(d_r)
        b += k
    assert b == d_in.shape[0]
    torch.cuda.synchronize()
    p, r = torch.cat(ps).cpu().numpy(), torch.cat(rs).cpu().numpy()
    assert not np.any(p == PERIOD_SENTINEL) and not np.any(np.isnan(r))
    return p, r


def _tracker(c, hold=None, glide=None):
    from vocoderproject_amd import StreamingPitchTracker
    return StreamingPitchTracker(len(c.signals), c.N, c.fs, c.F, hold_blocks=c.hold if hold is None else hold, glide=c.glide if glide is None else glide)


# ---- 1. the batch kernel on every edge case --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", EC.CASES, ids=EC.case_id)
def test_period_and_ratio_equal_the_reference_bit_for_bit(c):
    from vocoderproject_amd import StftRoundTrip
    ref_p, ref_r, _ = EC.reference(c)
    for s in range(EC.N_STREAMS):
        assert EC.holds(c, s), (c.name, s)                                           # (the case is what it is there for)
    st = StftRoundTrip(EC.N_STREAMS, EC.length(c), c.F, c.hop)
    p, r = _raw_track(st, _dev(EC.batch_input(c), np.float32), c.fs, _dev(c.keys, np.int32))
    st.close()
    _same(p, r, ref_p, ref_r)


def test_many_streams_with_a_partial_last_workgroup():
    from vocoderproject_amd import StftRoundTrip
    x, keys, ref_p, ref_r = EC.many_input()
    S, T = x.shape
    src = EC.MANY_SOURCES[0]
    st = StftRoundTrip(S, T, src.F, src.hop)
    assert S == EC.MANY_S and (S * st.n_frames) % EC.VP_TRACK_WAVES != 0
    p, r = _raw_track(st, _dev(x, np.float32), src.fs, _dev(keys, np.int32))
    st.close()
    _same(p, r, ref_p, ref_r)                                                        # every row: its three-stream result


# ---- 2. the streaming kernels ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", EC.STREAM_CASES, ids=SC.case_id)
def test_streaming_equals_the_reference_in_every_grouping(c):
    ref_p, ref_r, _ = EC.stream_reference(c)
    d_in, d_key = _dev(EC.stream_input(c), np.float32), _dev(c.keys, np.int32)
    for name, groups in EC.stream_groupings(c).items():
        trk = _tracker(c)
        p, r = _feed(trk, d_in, groups, d_key)
        trk.close()
        try:
            _same(p, r, ref_p, ref_r)
        except AssertionError as e:
            raise AssertionError(f"{c.name} grouping {name} {groups[:8]}: {e}") from None


@pytest.mark.parametrize("c", [EC.STREAM_BY_N[k] for k in ((44100, 1024, 1), (44100, 1024, 24), (44100, 1024, 65))], ids=SC.case_id)
def test_raw_decision_equals_the_batch_kernel_on_the_window(c):
    """H = 0, g = 1: block b's ratio (n_b >= W) is vp_stft_track_pitch's for the row x[n_b - W, n_b) on the same GPU; the calls are cut so
    that the windows of the compared blocks mix ring and slab."""
    from vocoderproject_amd import StftRoundTrip
    x = EC.stream_input(c)
    S, W, fd = len(c.signals), SC.window(c), SC.first_decision(c)
    trk = _tracker(c, hold=0, glide=1.0)
    p, r = _feed(trk, _dev(x, np.float32), EC.stream_groupings(c)["below-W"], _dev(c.keys, np.int32))
    trk.close()
    rows = SC.rows(x)
    assert np.all(p[:fd] == 0) and np.all(r[:fd] == 1.0)
    wins = np.concatenate([rows[:, (b + 1) * c.N - W:(b + 1) * c.N] for b in range(fd, c.n_blocks)])
    st = StftRoundTrip(wins.shape[0], W, c.F, c.F // 2)                              # (rows of W samples: frame 0 reads the whole row)
    bp, br = _raw_track(st, _dev(wins, np.float32), c.fs, _dev(list(c.keys) * (c.n_blocks - fd), np.int32))
    st.close()
    _same(p[fd:], r[fd:], bp[:, 0].reshape(-1, S), br[:, 0].reshape(-1, S))
    assert np.any(p[fd:] > 0)


# ---- 3. the autotune entry points on top-of-range input ------------------------------------------------------------------------------------------------
def test_stft_autotune_on_a_top_case_is_the_tracker_then_the_curve_call():
    from vocoderproject_amd import StftRoundTrip
    c = EC.BY_NAME["top-fs44100-F1024-p55"]
    ref_p, ref_r, d = EC.reference(c)
    assert np.all(d["idx"] == d["notesN"]) and np.any(ref_r > 1.0)
    st = StftRoundTrip(EC.N_STREAMS, EC.length(c), c.F, c.hop)
    d_in, d_key = _dev(EC.batch_input(c), np.float32), _dev(c.keys, np.int32)
    p, r = _raw_track(st, d_in, c.fs, d_key)
    _same(p, r, ref_p, ref_r)
    d_parts = torch.full_like(d_in, float("nan"))
    st.pitch_shift_curve(d_in, d_parts, d_ratio=_dev(r, np.float64))
    d_out = torch.full_like(d_in, float("nan"))
    d_p = torch.full((st.S, st.n_frames), PERIOD_SENTINEL, dtype=torch.int32, device="cuda")
    d_r = torch.full((st.S, st.n_frames), float("nan"), dtype=torch.float64, device="cuda")
    rc = st.L.vp_stft_autotune(st.h, d_in.data_ptr(), d_out.data_ptr(), c.fs, d_key.data_ptr(), d_p.data_ptr(), d_r.data_ptr(),
                               C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    st.close()
    assert rc == 0
    y, y_parts = d_out.cpu().numpy(), d_parts.cpu().numpy()
    assert np.all(np.isfinite(y)) and np.abs(y).max() > 0.1
    assert np.array_equal(y.view(np.uint32), y_parts.view(np.uint32))
    _same(d_p.cpu().numpy(), d_r.cpu().numpy(), ref_p, ref_r)


def test_streaming_autotune_on_a_top_case_is_the_tracker_then_the_curve_call():
    from vocoderproject_amd import PhaseVocoderStream
    c = EC.STREAM_BY_N[(44100, 1024, 24)]
    S, hop = len(c.signals), 256
    ref_p, ref_r, _ = EC.stream_reference(c)
    d_in, d_key = _dev(EC.stream_input(c), np.float32), _dev(c.keys, np.int32)
    groups = EC.stream_groupings(c)["mixed"]
    outs, tables = [], []
    for one_call in (False, True):
        trk, pv = _tracker(c), PhaseVocoderStream(S, c.N, hop)
        d_out = torch.full_like(d_in, float("nan"))
        ps, rs, b = [], [], 0
        for k in groups:
            if one_call:
                d_p = torch.full((k, S), PERIOD_SENTINEL, dtype=torch.int32, device="cuda")
                d_r = torch.full((k, S), float("nan"), dtype=torch.float64, device="cuda")
                rc = pv.L.vp_pv_autotune_blocks_device(pv.h, trk.h, d_in[b:b + k].data_ptr(), d_out[b:b + k].data_ptr(), d_key.data_ptr(),
                                                       d_p.data_ptr(), d_r.data_ptr(), k, C.c_void_p(torch.cuda.current_stream().cuda_stream))
                assert rc == 0
            else:
                d_p, d_r = _call(trk, d_in[b:b + k], d_key)
                pv.process_device(d_in[b:b + k], d_out[b:b + k], n_blocks=k, d_ratio=d_r)
            ps.append(d_p)
            rs.append(d_r)
            b += k
        torch.cuda.synchronize()
        trk.close()
        pv.close()
        outs.append(d_out.cpu().numpy())
        tables.append((torch.cat(ps).cpu().numpy(), torch.cat(rs).cpu().numpy()))
    for p, r in tables:
        _same(p, r, ref_p, ref_r)
    top = [s for s, sp in enumerate(c.signals) if sp[0] == "sine_p"]
    assert top and np.all(ref_r[-1, top] > 1.0)                                       # (the popped slot, returned in key 7)
    assert np.all(np.isfinite(outs[0])) and np.abs(outs[0]).max() > 0.1
    assert np.array_equal(outs[1].view(np.uint32), outs[0].view(np.uint32))
