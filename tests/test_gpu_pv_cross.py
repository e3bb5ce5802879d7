"""The cross-synthesis kernels (vp_k_stft_cross, vp_k_xs_stream; csrc/vp_stft_cross.inc) on the GPU against the NumPy definition
(tests/pv_cross_reference.py) on every case of tests/pv_cross_cases.py, held to the plain round trip's gate
|y - ref| <= 3e-7 max(1, max |ref|) per stream; the identities (depth 0 is vp_stft_roundtrip of the carrier bit for bit), the run
partition, the streaming form against the one-shot bit for bit, resets, allocation counts, 300 streams and the argument errors.
tests/test_gpu_parity.py reruns this file with the whole GPU suite on the VP_POISON_LDS twin."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: the process then has one HIP runtime, torch's)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pv_cross_cases as XC  # noqa: E402
import pv_cross_reference as XR  # noqa: E402

pytestmark = pytest.mark.gpu

S, F = XC.N_STREAMS, XC.F
VP_ERR_INVALID_ARG, VP_ERR_GEOMETRY = -1, -4              # include/vp_amd.h


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _cur():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cross(st, v, c, depth=None, nc=32):
    """One vp_stft_cross_synth call on v, c [S][T] (depth None: the NULL table); the output starts as NaN, so every sample must have been
    written."""
    d_v, d_c = _dev(v, np.float32), _dev(c, np.float32)
    d_out = torch.full_like(d_c, float("nan"))
    d_d = _dev(depth, np.float64) if depth is not None else None
    rc = st.L.vp_stft_cross_synth(st.h, d_v.data_ptr(), d_c.data_ptr(), d_out.data_ptr(), d_d.data_ptr() if d_d is not None else None, int(nc), _cur())
    torch.cuda.synchronize()
    assert rc == 0, (rc, st.L.vp_stft_last_error(st.h))
    return d_out.cpu().numpy()


def _roundtrip(st, x):
    d_in = _dev(x, np.float32)
    d_out = torch.full_like(d_in, float("nan"))
    st(d_in, d_out)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def _blocks(x, N):
    n, T = x.shape
    return _dev(x.reshape(n, T // N, N).transpose(1, 0, 2), np.float32)


def _rows(d):
    nb, n, N = d.shape
    return d.cpu().numpy().transpose(1, 0, 2).reshape(n, nb * N)


def _stream(xs, v, c, group, depth=None, nc=32, reset_at=None):
    """v, c [n][T] through the handle, `group` blocks per call; reset_at: (block, stream) -- vp_xs_reset(stream) in front of the call that
    starts with that block.  -> [n][T]; the allocation count must not move."""
    d_v, d_c = _blocks(v, xs.N), _blocks(c, xs.N)
    d_out = torch.full_like(d_v, float("nan"))
    d_d = _dev(depth, np.float64) if depth is not None else None
    nb = d_v.shape[0]
    allocs = xs.debug_alloc_count()
    b = 0
    while b < nb:
        k = min(group, nb - b)
        if reset_at is not None and reset_at[0] == b:
            xs.reset(reset_at[1])
        rc = xs.L.vp_xs_process_blocks_device(xs.h, d_v[b:b + k].data_ptr(), d_c[b:b + k].data_ptr(), d_out[b:b + k].data_ptr(),
                                              d_d.data_ptr() if d_d is not None else None, int(nc), k, _cur())
        assert rc == 0, rc
        assert xs.debug_alloc_count() == allocs
        b += k
    torch.cuda.synchronize()
    return _rows(d_out)


# ---- 1. one-shot against NumPy ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", XC.CASES, ids=XC.case_id)
def test_one_shot_cross_synthesis_matches_numpy(c):
    from vocoderproject_amd import StftRoundTrip
    (v, x), ref = XC.case_input(c), XC.reference(c)
    T = XC.length(c)
    st = StftRoundTrip(S, T, F, c.hop)
    y = _cross(st, v, x, XC.depths(c), c.nc)
    st.close()
    assert np.all(np.isfinite(y))
    for s in range(S):
        err, bnd = np.abs(y[s] - ref[s]).max(), XC.gate(ref[s])
        print(f"CROSS {XC.case_id(c)} stream {s}: err {err:.3g} gate {bnd:.3g}")
        assert err <= bnd, (s, err, bnd)
    covered = (st.n_frames - 1) * c.hop + F
    assert np.all(y[:, covered:] == 0) and (c.length != "uncovered" or T - covered == 37)       # samples no frame covers


def test_the_python_entry_makes_the_same_call():
    from vocoderproject_amd import StftRoundTrip
    c = XC.CrossCase(256, "tail", 32, True)
    v, x = XC.case_input(c)
    st = StftRoundTrip(S, XC.length(c), F, c.hop)
    d_v, d_c = _dev(v, np.float32), _dev(x, np.float32)
    outs = []
    for kw in (dict(depth=XC.DEPTHS), dict(d_depth=_dev(XC.DEPTHS, np.float64)), dict(depth=None), dict()):
        d_out = torch.full_like(d_c, float("nan"))
        st.cross_synth(d_v, d_c, d_out, lifter=c.nc, **kw)
        torch.cuda.synchronize()
        outs.append(d_out.cpu().numpy())
    assert np.array_equal(outs[0], _cross(st, v, x, XC.DEPTHS, c.nc)) and np.array_equal(outs[1], outs[0])
    assert np.array_equal(outs[2], _cross(st, v, x, None, c.nc)) and np.array_equal(outs[3], outs[2])       # the default depth 1.0 is the NULL table's
    st.close()


# ---- 2. the identities ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", XC.HOPS)
def test_depth_zero_is_bit_identical_to_the_round_trip_of_the_carrier(hop):
    from vocoderproject_amd import StftRoundTrip
    T = F + 11 * hop + 37
    v, x = XC.signals(T, seed=hop)
    st = StftRoundTrip(S, T, F, hop)
    plain = _roundtrip(st, x)
    for depth in (np.zeros(S), np.array([-0.0, -2.0, float("nan")])):                 # (fmax first: a NaN is 0)
        assert np.array_equal(_cross(st, v, x, depth, 32), plain)
    st.set_precision("f32")                                                           # always double, whatever the handle's precision says
    assert np.array_equal(_cross(st, v, x, np.zeros(S), 4), plain)
    st.set_precision("f64")
    # voice == carrier: ev and ec come out of the same instructions on the same data at different times -- held to the gate
    y = _cross(st, x, x, None, 32)
    full = _cross(st, v, x, None, 32)
    st.close()
    for s in range(S):
        err, bnd = np.abs(y[s] - plain[s].astype(np.float64)).max(), XC.gate(plain[s])
        print(f"CROSS voice == carrier hop {hop} stream {s}: err {err:.3g} gate {bnd:.3g}")
        assert err <= bnd, (s, err, bnd)
    assert not np.array_equal(full, plain)


# ---- 3. runs ------------------------------------------------------------------------------------------------------------------------------------
def test_the_run_partition_changes_no_bit():
    from vocoderproject_amd import StftRoundTrip
    T = 1024 + 48 * 256
    v, x = XC.signals(T, seed=3)
    st = StftRoundTrip(S, T, F, 256)
    outs = []
    for runs in (1, 3, 0):
        st.set_runs(runs)
        outs.append(_cross(st, v, x, XC.DEPTHS, 32))
    st.close()
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
    ref = XR.cross_synth(v[0], x[0], F, 256, 1.0, 32)
    assert np.abs(outs[0][0] - ref).max() <= XC.gate(ref)


# ---- 4. streaming -------------------------------------------------------------------------------------------------------------------------------
# (+ hop 128, which XC.STREAM_CASES compare with the one-shot at no block size)
@pytest.mark.parametrize("c", XC.STREAM_CASES + [XC.StreamCase(256, 128, 20, 32)], ids=XC.stream_id)
def test_streaming_is_bit_identical_to_the_one_shot_and_grouping_changes_no_bit(c):
    from vocoderproject_amd import CrossSynthStream, StftRoundTrip
    v, x = XC.stream_input(c)
    T = c.N * c.n_blocks
    st = StftRoundTrip(S, T, F, c.hop)
    one = _cross(st, v, x, XC.DEPTHS, c.nc)
    st.close()
    outs = []
    for group in XC.STREAM_GROUPS:
        xs = CrossSynthStream(S, c.N, hop=c.hop)
        L = xs.latency
        assert L == F - int(np.gcd(c.N, c.hop))
        outs.append(_stream(xs, v, x, group, XC.DEPTHS, c.nc))
        xs.close()
    assert np.all(outs[0][:, :L] == 0) and np.array_equal(outs[0][:, L:], one[:, :T - L])
    assert np.array_equal(outs[1], outs[0]) and np.array_equal(outs[2], outs[0])
    ref = XR.cross_synth(v[1], x[1], F, c.hop, 0.5, c.nc)
    assert np.abs(outs[0][1, L:] - ref[:T - L]).max() <= XC.gate(ref)


def test_a_reset_restarts_that_stream_only():
    from vocoderproject_amd import CrossSynthStream
    c = XC.StreamCase(256, 128, 24, 32)
    v, x = XC.stream_input(c)
    xs = CrossSynthStream(S, c.N, hop=c.hop)
    plain = _stream(xs, v, x, 3)
    xs.reset()                                                                         # every stream: the same output again
    assert np.array_equal(_stream(xs, v, x, 3), plain)
    xs.reset(-1)
    y = _stream(xs, v, x, 3, reset_at=(9, 1))
    xs.close()
    assert np.array_equal(y[0], plain[0]) and np.array_equal(y[2], plain[2])
    cut = 9 * c.N
    assert np.array_equal(y[1, :cut], plain[1, :cut])
    fresh = CrossSynthStream(S, c.N, hop=c.hop)                                        # stream 1 from block 9 on equals a fresh stream's output
    tail = _stream(fresh, v[:, cut:], x[:, cut:], 3)
    fresh.close()
    assert np.array_equal(y[1, cut:], tail[1]) and not np.array_equal(y[1, cut:], plain[1, cut:])


def test_more_pending_resets_than_a_call_carries_and_three_hundred_streams():
    from vocoderproject_amd import CrossSynthStream, StftRoundTrip
    n, N, nb = XC.BIG_S, XC.BIG_N, XC.BIG_BLOCKS
    v, x = XC.big_input()
    xs = CrossSynthStream(n, N, hop=XC.BIG_HOP)
    L = xs.latency
    first = _stream(xs, v, x, 2)
    for s in range(0, n, 2):                                                           # 150 pending resets: update launches in front of the call
        xs.reset(s)
    again = _stream(xs, v, x, nb)
    xs.close()
    assert np.array_equal(again[0::2], first[0::2])                                    # the reset streams start over ...
    assert not np.array_equal(again[1::2], first[1::2])                                # ... the others went on
    st = StftRoundTrip(n, N * nb, F, XC.BIG_HOP)
    one = _cross(st, v, x, None, 32)
    st.close()
    assert np.all(first[:, :L] == 0) and np.array_equal(first[:, L:], one[:, :N * nb - L])
    for s in (0, 1, 2, 149, 299):
        ref = XR.cross_synth(v[s], x[s], F, XC.BIG_HOP, None, 32)
        err, bnd = np.abs(one[s] - ref).max(), XC.gate(ref)
        print(f"CROSS big stream {s}: err {err:.3g} gate {bnd:.3g}")
        assert err <= bnd, (s, err, bnd)


def test_the_stream_runner_aligns_its_output_with_its_input():
    from vocoderproject_amd import CrossSynthStream
    T = 3000
    v, x = XC.signals(T, seed=5)
    xs = CrossSynthStream(S, 256, hop=128)
    y = xs.run(v, x, blocks_per_call=5, depth=XC.DEPTHS, lifter=32)
    xs.close()
    assert y.shape == (S, T) and y.dtype == np.float32
    for s in range(S):
        # the runner pads with zeros: frames that start at or before T - F + (padding) exist, so compare against the padded one-shot
        pad = np.zeros(T + 2048)
        pv, px = pad.copy(), pad.copy()
        pv[:T], px[:T] = v[s], x[s]
        ref = XR.cross_synth(pv, px, F, 128, XC.DEPTHS[s], 32)[:T]
        assert np.abs(y[s] - ref).max() <= XC.gate(ref), s


# ---- 5. silence -----------------------------------------------------------------------------------------------------------------------------------
def test_silent_inputs_stay_finite_and_a_silent_carrier_gives_zeros():
    from vocoderproject_amd import StftRoundTrip
    T = F + 5 * 256
    v, x = XC.signals(T)
    z = np.zeros_like(v)
    st = StftRoundTrip(S, T, F, 256)
    quiet = _cross(st, z, x, None, 32)                                                 # a silent voice silences the carrier: no lower clamp
    assert np.all(np.isfinite(quiet)) and np.abs(quiet[0]).max() < 1e-3 * np.abs(x[0]).max()
    ref = XR.cross_synth(z[0], x[0], F, 256, None, 32)
    assert np.abs(quiet[0] - ref).max() <= XC.gate(ref)
    assert np.all(_cross(st, v, z, None, 32) == 0) and np.all(_cross(st, z, z, None, 32) == 0)
    st.close()


# ---- 6. argument errors -----------------------------------------------------------------------------------------------------------------------
def test_argument_errors_are_reported_before_the_device_is_touched():
    from vocoderproject_amd import CrossSynthStream, StftRoundTrip, VpError
    T = 4096
    v, x = XC.signals(T)
    v, x = v[:2], x[:2]
    st, st2k = StftRoundTrip(2, T, 1024, 256), StftRoundTrip(2, T, 2048, 512)
    d_v, d_c = _dev(v, np.float32), _dev(x, np.float32)
    d_out = torch.full_like(d_c, float("nan"))
    d_d = _dev(np.ones(2), np.float64)
    i, c, o, d = d_v.data_ptr(), d_c.data_ptr(), d_out.data_ptr(), d_d.data_ptr()

    def neighbours():
        o1, o2 = torch.full_like(d_c, float("nan")), torch.full_like(d_c, float("nan"))
        st(d_c, o1)
        st.pitch_shift(d_c, o2, -5.0)
        torch.cuda.synchronize()
        return o1.cpu().numpy(), o2.cpu().numpy()
    before = neighbours()
    good = _cross(st, v, x, np.ones(2), 32)
    call = st.L.vp_stft_cross_synth
    for args in ((None, c, o, d, 32), (i, None, o, d, 32), (i, c, None, d, 32), (i, c, o, d, 3), (i, c, o, d, 65), (i, c, o, None, 0), (i, c, o, d, -1)):
        assert call(st.h, *args, _cur()) == VP_ERR_INVALID_ARG, args
        assert st.L.vp_stft_last_error(st.h).startswith(b"cross:")
    assert call(None, i, c, o, d, 32, _cur()) == VP_ERR_INVALID_ARG
    assert call(st2k.h, None, c, o, d, 32, _cur()) == VP_ERR_INVALID_ARG               # the pointers before the frame length
    assert call(st2k.h, i, c, o, d, 65, _cur()) == VP_ERR_INVALID_ARG                  # ... and the lifter
    assert call(st2k.h, i, c, o, d, 32, _cur()) == VP_ERR_GEOMETRY
    msg = st.L.vp_stft_last_error(st2k.h)
    assert msg.startswith(b"cross:") and b"2048-point frames are not built" in msg
    torch.cuda.synchronize()
    assert torch.all(torch.isnan(d_out))                                               # nothing ran
    with pytest.raises(VpError):
        st2k.cross_synth(d_v, d_c, d_out)
    with pytest.raises(ValueError):
        st.cross_synth(d_v, d_c, d_out, lifter=65)
    with pytest.raises(ValueError):
        st.cross_synth(d_v, d_c[:, :T - 1], d_out)
    with pytest.raises(ValueError):
        st.cross_synth(d_v.double(), d_c, d_out)
    with pytest.raises(ValueError):
        st.cross_synth(d_v, d_c, d_c)
    assert torch.all(torch.isnan(d_out))
    # a valid call afterwards still gives its bits, and the neighbours on the same handle theirs
    assert np.array_equal(_cross(st, v, x, np.ones(2), 32), good)
    for a, b in zip(before, neighbours()):
        assert np.array_equal(a, b)
    st.close()
    st2k.close()

    h = C.c_void_p()
    lib = st.L
    assert lib.vp_xs_create(0, 2, 256, 2048, 512, C.byref(h)) == VP_ERR_GEOMETRY and not h.value
    assert lib.vp_xs_create(0, 2, 256, 1024, 96, C.byref(h)) == VP_ERR_GEOMETRY and not h.value
    with pytest.raises(VpError):
        CrossSynthStream(2, 256, frame_len=2048, hop=512)
    N = 256
    xs = CrossSynthStream(2, N)
    b_v, b_c = _blocks(v[:, :4 * N], N), _blocks(x[:, :4 * N], N)
    b_out = torch.full_like(b_c, float("nan"))
    bi, bc, bo = b_v.data_ptr(), b_c.data_ptr(), b_out.data_ptr()
    call = lib.vp_xs_process_blocks_device
    for args in ((None, bc, bo, d, 32, 4), (bi, None, bo, d, 32, 4), (bi, bc, None, d, 32, 4), (bi, bc, bo, d, 3, 4), (bi, bc, bo, d, 65, 4), (bi, bc, bo, d, 32, 0),
                 (bi, bc, bo, d, 32, -1)):
        assert call(xs.h, *args, _cur()) == VP_ERR_INVALID_ARG, args
    assert call(None, bi, bc, bo, d, 32, 4, _cur()) == VP_ERR_INVALID_ARG
    assert lib.vp_xs_reset(xs.h, 2) == VP_ERR_INVALID_ARG and lib.vp_xs_reset(xs.h, -2) == VP_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert torch.all(torch.isnan(b_out))
    # the refused calls left the stream's state alone
    y = _stream(xs, v[:, :4 * N], x[:, :4 * N], 4)
    xs.close()
    fresh = CrossSynthStream(2, N)
    assert np.array_equal(y, _stream(fresh, v[:, :4 * N], x[:, :4 * N], 1))
    fresh.close()
