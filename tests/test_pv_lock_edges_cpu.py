"""The peak-locked EDGE cases on the CPU (tests/pv_lock_edge_cases.py; no GPU): every case reaches the branch it names (predicates on the
definition's trace), passes the two-form gate and a conditioning probe; what the first matrix (tests/pv_lock_cases.py gpu_input x
GPU_CURVES) reaches of the same branches is pinned; every edge mutant of the definition is seen by a named case; and a Python
transcription of the kernels' integer arithmetic (pv_lock_bin, the nine ballots, pv_lock_mask, pv_lock_nearest of csrc/vp_stft_lock.inc)
is compared with the definition's nearest() -- a model, not a test of the kernel: its named faults predict which GPU cases see which
seeded kernel fault (profiles/pv_lock_mutations.txt).  Run with -s for the PVLOCKEDGE lines.

The conditioning probe moves every bin of every frame's spectrum by 1e-13 of the frame's largest magnitude -- a thousand times a double
FFT's rounding -- and reruns the first form; the output must move by less than 1 % of the case's GPU bound, on three seeds.  Bins 0 and N
are moved along the real axis only: the transform of a real frame leaves them real by construction, in NumPy and in the kernels
(rfft_split), so no rounding error ever gives them an imaginary part, and the half-turn unwrap tie there is the definition's rule
(tests/pv_lock_reference.py, the module's note), not a matter of conditioning."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pv_lock_cases as LC  # noqa: E402
import pv_lock_edge_cases as E  # noqa: E402
import pv_lock_reference as LR  # noqa: E402

F, N = LC.F, LC.F // 2
CONDITION_EPS, CONDITION_SEEDS, CONDITION_SHARE = 1e-13, (0, 1, 2), 0.01

# cases that miss the gate or the conditioning probe: properties only, counted toward no predicate (none today)
PROPERTIES_ONLY = ()
POINTWISE = [c for c in E.CASES if c.name not in PROPERTIES_ONLY]


# ---- 1. the trace changes no bit ---------------------------------------------------------------------------------------------------------------
def test_the_trace_changes_no_bit_of_the_96_gate_cases():
    for c in LC.GATE_CASES:
        x, r, tr = LC.gate_input(c), LC.curve(c.curve, c.nF, c.hop), []
        y = LR.locked_roundtrip(x, r, F, c.hop, trace=tr)
        assert np.array_equal(y, LC.gate_reference(c)), LC.gate_id(c)
        assert len(tr) == c.nF and all(set(t) == {"P", "own", "Ps", "Pa", "owns", "r", "silent", "gone", "tie"} for t in tr)


def test_the_streaming_reference_hands_its_trace_through():
    c = E.STREAM_CASES[1]
    x, tab = E.stream_input(c), E.stream_ratios(c)
    tr = []
    y = LR.by_block(x[0], c.N, c.hop, tab[:, 0], trace=tr)
    assert np.array_equal(y, LR.by_block(x[0], c.N, c.hop, tab[:, 0])) and len(tr) == (len(x[0]) - F) // c.hop + 1


# ---- 2. gate, conditioning, predicates -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", E.CASES, ids=lambda c: c.name)
def test_every_case_passes_the_gate_is_well_conditioned_and_reaches_its_branch(c):
    y, tr = E.reference(c)
    yb, _ = E.reference(c, "b")
    scale = max(1.0, float(np.abs(y).max()))
    gate = np.abs(y - yb).max() / scale
    bnd = LC.bound(c.hop, y)
    x, r = E.case_input(c), E.case_ratios(c)
    moved = max(np.abs(LR.locked_roundtrip(x, r, F, c.hop, perturb=(CONDITION_EPS, s)) - y).max() for s in CONDITION_SEEDS)
    print(f"PVLOCKEDGE cpu {c.name}: gate {gate:.3g} moved {moved / bnd:.3g} of the bound, max |ref| {np.abs(y).max():.3g}")
    assert np.abs(y).max() > 100.0 * bnd or all(t["silent"] or t["gone"] for t in tr), c.name            # the comparison is not vacuous
    if c.name in PROPERTIES_ONLY:
        assert np.all(np.isfinite(y))
        return
    assert gate <= LC.GATE_TOL, (c.name, gate)
    assert moved < CONDITION_SHARE * bnd, (c.name, moved, bnd)
    for pred, arg in c.expect:
        n = E.count(c, pred, arg)
        print(f"PVLOCKEDGE cpu {c.name}: {pred}({arg}) on {n} frames")
        assert n >= 1, (c.name, pred, arg)


@pytest.mark.parametrize("c", E.STREAM_CASES, ids=E.stream_id)
def test_every_streaming_case_passes_the_gate_and_is_well_conditioned(c):
    """The streaming cases are the one-shot's frames with the per-frame table (asserted below): gated and probed in that form."""
    x, tab = E.stream_input(c), E.stream_ratios(c)
    per_frame = LC.per_frame(tab, c.N, c.hop, x.shape[1])
    for s in range(E.N_STREAMS):
        y = LR.locked_roundtrip(x[s], per_frame[s], F, c.hop)
        gate = np.abs(y - LR.locked_roundtrip_b(x[s], per_frame[s], F, c.hop)).max() / max(1.0, float(np.abs(y).max()))
        bnd = LC.bound(c.hop, y)
        moved = max(np.abs(LR.locked_roundtrip(x[s], per_frame[s], F, c.hop, perturb=(CONDITION_EPS, k)) - y).max() for k in CONDITION_SEEDS)
        print(f"PVLOCKEDGE cpu stream {E.stream_id(c)} pattern {s}: gate {gate:.3g} moved {moved / bnd:.3g} of the bound, max |ref| {np.abs(y).max():.3g}")
        assert gate <= LC.GATE_TOL, (s, gate)
        assert moved < CONDITION_SHARE * bnd, (s, moved, bnd)


def test_every_required_branch_is_reached_by_a_pointwise_case():
    assert len(E.GROUPS) <= 12 and all(len(v) <= 8 for v in E.GROUPS.values())
    assert {c.hop for c in E.CASES} >= {64, 512} and all(c.nF <= 16 and c.hop in LC.GPU_HOPS for c in E.CASES)
    for pred, arg in E.REQUIRED:
        n = {c.name: E.count(c, pred, arg) for c in POINTWISE}
        total = sum(n.values())
        print(f"PVLOCKEDGE reach {pred}({arg}): {total} frames in {sum(v > 0 for v in n.values())} cases")
        assert total >= 1, (pred, arg)
        assert any(v > 0 and (pred, arg) in c.expect for c, v in ((c, n[c.name]) for c in POINTWISE)), (pred, arg)   # and a case names it


def test_the_streaming_cases_reach_every_call_edge():
    assert all(c.N in (17, 100, 256, 1000) and c.hop in (64, 128, 512) for c in E.STREAM_CASES) and E.N_STREAMS <= 6
    assert {c.N for c in E.STREAM_CASES} == {17, 100, 256, 1000}
    total = dict.fromkeys(E.STREAM_REQUIRED, 0)
    for c in E.STREAM_CASES:
        n = E.stream_counts(c)
        print(f"PVLOCKEDGE stream reach {E.stream_id(c)}: {n}")
        for k, v in n.items():
            total[k] += v
    assert all(v >= 1 for v in total.values()), total
    # the block-by-block form under the call spans is the one-shot's frames with the per-frame table
    c = E.STREAM_CASES[1]
    y, _, _ = E.stream_reference(c)
    x, tab = E.stream_input(c), E.stream_ratios(c)
    L = LR.P.latency(c.N, c.hop)
    for s in range(E.N_STREAMS):
        one = LR.locked_roundtrip(x[s], LC.per_frame(tab, c.N, c.hop, x.shape[1])[s], F, c.hop)
        n = ((x.shape[1] - F) // c.hop + 1) * c.hop - L
        assert np.abs(y[s, L:L + n] - one[:n]).max() <= 1e-12


# ---- 3. what the first matrix reaches: pinned ------------------------------------------------------------------------------------------------------
_MATRIX = {}


def _matrix():
    """{(hop, nF, curve, stream): (y, trace)} of the first matrix, once."""
    if not _MATRIX:
        for hop in LC.GPU_HOPS:
            for nF in LC.GPU_NF:
                x = LC.gpu_input(hop, nF)
                for name in LC.GPU_CURVES:
                    r = LC.gpu_ratios(name, hop, nF)
                    for s in range(len(x)):
                        tr = []
                        _MATRIX[hop, nF, name, s] = (LR.locked_roundtrip(x[s], r[s], F, hop, trace=tr), tr)
    return _MATRIX


MATRIX_PINNED = {("silent_at", 0): 0, ("silent_at", 1): 0, ("silent_at", 2): 0, ("silent_at", 3): 0, ("any_silent", None): 0, ("any_gone", None): 0}


def test_what_the_first_matrix_reaches_is_pinned():
    m = _matrix()
    frames = [t for _, tr in m.values() for t in tr]
    assert len(m) == 864 and len(frames) == 4176
    got = {}
    for pred, arg in list(E.REQUIRED) + [("any_silent", None), ("any_gone", None)]:
        if pred == "gone_raw":
            continue                                                                  # (no frame is gone: nothing to look the raw ratio up for)
        got[pred, arg] = sum(E.PREDICATES[pred](None, tr, arg) for _, tr in m.values())
    lowest = max(int(t["P"][0]) for t in frames)
    on_n = sum(N in E._shifted(t) for t in frames)
    ties = sum(bool(t["tie"]) for _, tr in m.values() for t in tr[1:])                     # (between consecutive frames: not frame 0 against the zero state)
    print(f"PVLOCKEDGE matrix: largest lowest peak {lowest}, frames with P' == N {on_n}, unwrap ties {ties}")
    for k, v in got.items():
        print(f"PVLOCKEDGE matrix {k[0]}({k[1]}): {v}")
    assert lowest == 23 and on_n == 262 and ties == 504 and sum(bool(t["tie"]) for t in frames) == 696
    for k, v in MATRIX_PINNED.items():
        assert got[k] == v, (k, got[k])
    for k in (("last_silent", None), ("silent_between", None), ("silent_rounds", None), ("gone_then_used", None), ("lowest_word", 1),
              ("lowest_word", 2), ("lowest_word", 8), ("highest_le", 0), ("single_at", 512), ("single_at", 256), ("single_mod63", None),
              ("double_lowest_ge_128", None)):
        assert got[k] == 0, (k, got[k])                                               # the gap the edge cases close


# ---- 4. the edge mutants ---------------------------------------------------------------------------------------------------------------------------
EDGE_TEETH = {"silent_theta": "gap-hop512-in2-nF7", "silent_prev": "gap-hop512-in2-nF7", "gone_theta": "gone-hop512", "drop_n": "edge15-hop512",
              "no_lower": "word1-hop512", "near_only": "tie0-hop512", "top_lost": "gone512-hop512"}
# the (hop, nF, curve, stream) cases of the first matrix, of 864, that each mutant moves by more than the GPU bound (measured; pinned)
MATRIX_CHANGED = {"silent_theta": 0, "silent_prev": 0, "gone_theta": 0, "drop_n": 133, "no_lower": 816, "near_only": 432, "top_lost": 220}


@pytest.mark.parametrize("mutant", LR.EDGE_MUTANTS)
def test_every_edge_mutant_is_seen_by_a_named_edge_case(mutant):
    assert set(EDGE_TEETH) == set(LR.EDGE_MUTANTS) and all(v not in PROPERTIES_ONLY for v in EDGE_TEETH.values())
    c = E.BY_NAME[EDGE_TEETH[mutant]]
    y, _ = E.reference(c)
    ym, _ = E.reference(c, "a", mutant)
    away = np.abs(ym - y).max() / LC.bound(c.hop, y)
    seen = [k.name for k in POINTWISE if np.abs(E.reference(k, "a", mutant)[0] - E.reference(k)[0]).max() > LC.bound(k.hop, E.reference(k)[0])]
    print(f"PVLOCKEDGE mutant {mutant}: {away:.3g} bounds away on {c.name}; changes {len(seen)} of {len(POINTWISE)} edge cases")
    assert away >= LC.TEETH, (mutant, away)
    changed = 0
    for (hop, nF, name, s), (y0, _) in _matrix().items():
        x, r = LC.gpu_input(hop, nF)[s], LC.gpu_ratios(name, hop, nF)[s]
        changed += bool(np.abs(LR.locked_roundtrip(x, r, F, hop, mutant) - y0).max() > LC.bound(hop, y0))
    print(f"PVLOCKEDGE mutant {mutant}: changes {changed} of {len(_matrix())} cases of the first matrix")
    assert changed == MATRIX_CHANGED[mutant], (mutant, changed)


def test_every_ownership_tie_case_shows_how_its_tie_resolves():
    """A case that names an ownership tie must carry it into the output: with the tie given to the upper peak (the first mutants'
    `tieup`) it is at least TEETH bounds away.  (Below ratio 1 the sources of two shifted regions leave a gap around the middle bin and
    its owner is never read: the tie cases run above 1.)"""
    cases = [c for c in POINTWISE if any(p == "own_tie_at" for p, _ in c.expect)]
    assert {a for c in cases for p, a in c.expect if p == "own_tie_at"} == {63, 0} and len(cases) >= 4
    for c in cases:
        y = E.reference(c)[0]
        away = np.abs(E.reference(c, "a", "tieup")[0] - y).max() / LC.bound(c.hop, y)
        print(f"PVLOCKEDGE mutant tieup: {away:.3g} bounds away on {c.name}")
        assert away >= LC.TEETH, (c.name, away)


# ---- 5. the kernels' integer arithmetic, transcribed -------------------------------------------------------------------------------------------------
M64 = (1 << 64) - 1
MODEL_FAULTS = ("no_below_bit", "w8_zero", "down_if", "up_j7", "tie_lt")           # faults 1 .. 5 of profiles/pv_lock_mutations.txt


def k_bin(e, lane):
    return 256 if e == 8 else (512 - (64 * (e >> 1) + lane)) if e & 1 else 64 * (e >> 1) + lane


def k_ballots(flag):
    """flag: bool [513] -> the nine ballots (bit `lane` of ballot e: the flag of bin k_bin(e, lane); e = 8: lane 0 only)."""
    bal = [0] * 9
    for e in range(9):
        for lane in range(64 if e < 8 else 1):
            if flag[k_bin(e, lane)]:
                bal[e] |= 1 << lane
    return bal


def _bitreverse64(x):
    return int(format(x, "064b")[::-1], 2)


def k_mask(bal, fault=None):
    W = [0] * 9
    for q in range(4):
        W[q] = bal[2 * q]
    for q in range(4):
        below = bal[2 * q + 3] if q < 3 else bal[8]
        W[7 - q] = ((_bitreverse64(bal[2 * q + 1]) << 1) & M64) | (0 if fault == "no_below_bit" else below & 1)
    W[8] = 0 if fault == "w8_zero" else bal[1] & 1
    return W


def k_nearest(W, k, fault=None):
    wi, b = k >> 6, k & 63
    w0 = W[wi]
    x = w0 & (M64 >> (63 - b))
    j = wi
    if fault == "down_if":
        if x == 0 and j > 0:
            j -= 1
            x = W[j]
    else:
        while x == 0 and j > 0:
            j -= 1
            x = W[j]
    lo = 64 * j + x.bit_length() - 1 if x else -1
    x = 0 if b == 63 else w0 & ((M64 << (b + 1)) & M64)
    j = wi
    while x == 0 and j < (7 if fault == "up_j7" else 8):
        j += 1
        x = W[j]
    hi = 64 * j + (x & -x).bit_length() - 1 if x else -1
    if lo < 0:
        return hi
    if hi < 0:
        return lo
    return lo if ((k - lo < hi - k) if fault == "tie_lt" else (k - lo <= hi - k)) else hi


def k_owners(idx, fault=None):
    flag = np.zeros(N + 1, bool)
    flag[list(idx)] = True
    W = k_mask(k_ballots(flag), fault)
    return np.array([k_nearest(W, k, fault) for k in range(N + 1)])


def test_the_lane_to_bin_map_covers_every_bin_once():
    bins = sorted(k_bin(e, lane) for e in range(9) for lane in range(64 if e < 8 else 1))
    assert bins == list(range(N + 1))


def _edge_masks():
    out = {}
    for c in POINTWISE:
        for t in E.reference(c)[1]:
            for idx in (t["P"], t["Ps"]):
                if len(idx):
                    out.setdefault(tuple(int(v) for v in idx), c.name)
    for c in E.STREAM_CASES:
        for tr in E.stream_reference(c)[1]:
            for t in tr:
                for idx in (t["P"], t["Ps"]):
                    if len(idx):
                        out.setdefault(tuple(int(v) for v in idx), E.stream_id(c))
    return out


def test_the_transcribed_mask_and_search_are_the_definition_s_nearest():
    assert k_owners(()).tolist() == [-1] * (N + 1)                                    # the empty mask
    for b in range(N + 1):                                                            # every one-bit mask, every k
        assert np.array_equal(k_owners((b,)), LR.nearest([b], N + 1)), b
    edge = sorted({k for j in range(9) for k in (64 * j - 1, 64 * j, 64 * j + 1) if 0 <= k <= N})
    pairs = [(a, b) for i, a in enumerate(edge) for b in edge[i + 1:]]
    assert len(pairs) == 300
    for a, b in pairs:                                                                # both bits within one of a word boundary
        assert np.array_equal(k_owners((a, b)), LR.nearest([a, b], N + 1)), (a, b)
    masks = _edge_masks()
    print(f"PVLOCKEDGE model: {len(masks)} distinct masks from the edge cases")
    for idx in masks:
        assert np.array_equal(k_owners(idx), LR.nearest(list(idx), N + 1)), idx


def test_every_fault_of_the_model_differs_and_names_the_cases_that_see_it():
    masks = _edge_masks()
    for fault in MODEL_FAULTS:
        seen = sorted({name for idx, name in masks.items() if not np.array_equal(k_owners(idx, fault), LR.nearest(list(idx), N + 1))})
        print(f"PVLOCKEDGE model fault {fault}: wrong owners on masks of {len(seen)} cases: {', '.join(seen)}")
        assert seen, fault
