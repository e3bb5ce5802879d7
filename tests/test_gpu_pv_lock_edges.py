"""The peak-locked kernels (vp_k_stft_pv_lock, vp_k_pv_stream_lock of csrc/vp_stft_lock.inc) on the EDGE cases of
tests/pv_lock_edge_cases.py, whose branches, gate and conditioning tests/test_pv_lock_edges_cpu.py asserts on the CPU: frames without a
peak among sounding ones, frames whose peaks all shift past bin N, masks whose nearest set bit lies words away, ties on a word boundary,
P' == N beside P' == N + 1, sources outside 0 .. N, the half-turn unwrap tie; streaming calls that begin or end on a silent frame, hold
only silent frames or only frames that lose every peak, or hold no frame at all.  One-shot against the NumPy definition at every sample
(and exactly zero wherever the definition is exactly zero), streaming bit-identical to the one-shot.  The PVLOCKEDGE lines (-s) and the
seeded kernel faults these cases see are in profiles/pv_lock_mutations.txt."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: the process then has one HIP runtime, torch's)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pv_cases  # noqa: E402
import pv_lock_cases as LC  # noqa: E402
import pv_lock_edge_cases as E  # noqa: E402
import pv_lock_reference as LR  # noqa: E402

pytestmark = pytest.mark.gpu

F = LC.F


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _cur():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _one_shot(x, ratio, hop):
    """One vp_stft_pitch_shift_locked call on x [S][T] with a table of ratios [S][nF]; the output starts as NaN."""
    from vocoderproject_amd import StftRoundTrip
    st = StftRoundTrip(x.shape[0], x.shape[1], F, hop)
    assert st.n_frames == ratio.shape[1]
    d_in = _dev(x, np.float32)
    d_out = torch.full_like(d_in, float("nan"))
    d_ratio = _dev(ratio, np.float64)
    rc = st.L.vp_stft_pitch_shift_locked(st.h, d_in.data_ptr(), d_out.data_ptr(), d_ratio.data_ptr(), _cur())
    torch.cuda.synchronize()
    assert rc == 0, (rc, st.L.vp_stft_last_error(st.h))
    st.close()
    return d_out.cpu().numpy()


def _blocks(x, N):
    n, T = x.shape
    return _dev(x.reshape(n, T // N, N).transpose(1, 0, 2), np.float32)


def _rows(d):
    nb, n, N = d.shape
    return d.cpu().numpy().transpose(1, 0, 2).reshape(n, nb * N)


def _stream_locked(ps, d_in, d_tab, spans, b0=0, d_out=None):
    """Locked calls of `spans` blocks each from block b0 on; returns the device output [n_blocks][S][N] (NaN where no call wrote)."""
    if d_out is None:
        d_out = torch.full_like(d_in, float("nan"))
    for k in spans:
        rc = ps.L.vp_pv_process_blocks_locked_device(ps.h, d_in[b0:b0 + k].data_ptr(), d_out[b0:b0 + k].data_ptr(), d_tab[b0:b0 + k].data_ptr(), k, _cur())
        assert rc == 0, rc
        b0 += k
    return d_out


def _check(what, names, y, ref, hop, traces, shift=0):
    """Every sample within the bound; exactly zero where the definition is zero by construction (E.structural_zero)."""
    assert np.all(np.isfinite(y)), what
    for s, name in enumerate(names):
        err, bnd = np.abs(y[s] - ref[s]).max(), LC.bound(hop, ref[s])
        print(f"PVLOCKEDGE {what} stream {s} ({name}): err {err:.3g} bound {bnd:.3g} err/bound {err / bnd:.3f}")
        assert err <= bnd, (what, name, err, bnd)
        zero = E.structural_zero(traces[s], hop, len(ref[s]), shift)
        assert np.all(ref[s][zero] == 0) and np.all(y[s][zero] == 0), (what, name, int(np.count_nonzero(y[s][zero])))


# ---- 1. one-shot against NumPy ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(E.GROUPS), ids=E.group_id)
def test_one_shot_edge_cases_match_numpy(key):
    """The cases of one (hop, nF) stacked into one launch, every stream its own ratios."""
    cases, hop = E.GROUPS[key], key[0]
    x = np.stack([E.case_input(c) for c in cases])
    y = _one_shot(x, np.stack([E.case_ratios(c) for c in cases]), hop)
    ref = [E.reference(c)[0] for c in cases]
    _check(f"one-shot {E.group_id(key)}", [c.name for c in cases], y, ref, hop, [E.reference(c)[1] for c in cases])
    for s, c in enumerate(cases):                                                    # silent spans exist, and sound does
        tr = E.reference(c)[1]
        if all(t["silent"] or t["gone"] for t in tr):
            assert np.all(y[s] == 0)
        else:
            assert np.abs(y[s]).max() > 100.0 * LC.bound(hop, ref[s])


# ---- 2. streaming ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", E.STREAM_CASES, ids=E.stream_id)
def test_streaming_edge_cases_are_bit_identical_to_the_one_shot(c):
    from vocoderproject_amd import PhaseVocoderStream
    S, N, hop, nb = E.N_STREAMS, c.N, c.hop, c.n_blocks
    x, tab = E.stream_input(c), E.stream_ratios(c)
    T = x.shape[1]
    per_frame = LC.per_frame(tab, N, hop, T)
    y1 = _one_shot(x, per_frame, hop)
    k, x2 = E.further_blocks(c), E.further_input(c)                                  # the further call: one burst per stream, sounding
    d_in, d_tab = _blocks(np.concatenate([x, x2], axis=1), N), _dev(np.concatenate([tab, np.full((k, S), E.FURTHER_RATIO)]), np.float64)
    a = PhaseVocoderStream(S, N, hop=hop)
    d_a = _stream_locked(a, d_in, d_tab, pv_cases.call_spans(nb, LC.STREAM_CALLS))
    torch.cuda.synchronize()
    L = a.latency
    ya = _rows(d_a)[:, :T]
    n = min(per_frame.shape[1] * hop, T - L)                                         # finished one-shot samples that the stream has emitted
    assert n > 2 * F and np.all(ya[:, :L] == 0) and np.all(np.isfinite(ya))
    for s in range(S):
        assert np.array_equal(ya[s, L:L + n], y1[s, :n]), (s, np.abs(ya[s, L:L + n] - y1[s, :n]).max())
    ref, traces, _ = E.stream_reference(c)
    if N == 100:                                                                     # against the definition driven block by block
        ref = np.stack([LR.by_block(x[s], N, hop, tab[:, s]) for s in range(S)])
    _check(f"stream {E.stream_id(c)}", [f"pattern {s}" for s in range(S)], ya, ref, hop, traces, L)
    # another grouping leaves an equivalent record: the same bits before, and on a further, sounding call
    b = PhaseVocoderStream(S, N, hop=hop)
    d_b = _stream_locked(b, d_in, d_tab, pv_cases.call_spans(nb, (16, 1, 5)))
    _stream_locked(a, d_in, d_tab, [k], nb, d_a)
    _stream_locked(b, d_in, d_tab, [k], nb, d_b)
    torch.cuda.synchronize()
    a.close()
    b.close()
    ya, yb = _rows(d_a), _rows(d_b)
    assert np.array_equal(ya, yb), np.abs(ya - yb).max()
    assert np.all(np.isfinite(ya)) and all(np.abs(ya[s, T:]).max() > 1e-3 for s in range(S))
    # and the further call is the definition's: what silent and all-gone calls left in the record (theta advanced, the phases of the
    # last frame) is what the definition carries, not merely the same in both handles
    ref2, traces2, _ = E.stream_reference(c, further=True)
    _check(f"stream {E.stream_id(c)} with the further call", [f"pattern {s}" for s in range(S)], ya, ref2, hop, traces2, L)


@pytest.mark.parametrize("c", [E.STREAM_CASES[2], E.STREAM_CASES[0]], ids=E.stream_id)
def test_single_block_calls_hand_theta_and_the_phases_through_the_record(c):
    """A silent-heavy case one block per call: every frame's theta and previous phases come from the record.  hop 64 / N = 256 holds
    four frames in every call, among them silent and all-gone calls; hop 512 / N = 17 has calls without a frame behind a silent one and
    calls whose only frame is silent."""
    from vocoderproject_amd import PhaseVocoderStream
    S, N, hop, nb = E.N_STREAMS, c.N, c.hop, c.n_blocks
    x, tab = E.stream_input(c), E.stream_ratios(c)
    T = x.shape[1]
    per_frame = LC.per_frame(tab, N, hop, T)
    y1 = _one_shot(x, per_frame, hop)
    ps = PhaseVocoderStream(S, N, hop=hop)
    y = _rows(_stream_locked(ps, _blocks(x, N), _dev(tab, np.float64), [1] * nb))
    L = ps.latency
    ps.close()
    n = min(per_frame.shape[1] * hop, T - L)
    assert n > 2 * F and np.all(y[:, :L] == 0)
    for s in range(S):
        assert np.array_equal(y[s, L:L + n], y1[s, :n]), (s, np.abs(y[s, L:L + n] - y1[s, :n]).max())
    _check(f"single blocks {E.stream_id(c)}", [f"pattern {s}" for s in range(S)], y, E.stream_reference(c)[0], hop, E.stream_reference(c)[1], L)
