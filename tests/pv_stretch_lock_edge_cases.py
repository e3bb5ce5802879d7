"""The peak-locked time stretch's EDGE cases (vp_k_stft_pv_stretch_lock of csrc/vp_stft_stretch_lock.inc): tests/pv_lock_edge_cases.py's pass
over the written-out copy.  The copy's matrix (tests/pv_stretch_lock_cases.py) feeds it dense signals only, so the statements that were
copied by hand and then edited for the frame's advance D -- the early return of pv_stretch_lock_plan, the hand-over of the previous phases
and theta around a wavefront whose frame has no peak, the `kp <= N` store, the all-gone skip of the gather plan -- are never taken next to
a sounding frame, and never at an advance other than hop.  These cases take them: frames without a peak among sounding ones at every
wavefront slot, reached by a leap, a freeze, a reverse step and a clamped position; sounding frames directly behind a silent one at
D = 1, D = F, D clamped from above F, an odd D and D = 1000; frames whose peaks all shift past bin N at D != hop; the rotation factor
(r hop - D) / F negative, positive and exactly zero; the unwrap tie at bin N that an odd D makes without any sign flip, and the parent's
half-turn flips at D != hop; odd and even positions in one round of four wavefronts; P' == N beside P' == N + 1 and sources outside
0 .. N.  tests/test_pv_stretch_lock_edges_cpu.py asserts on the definition's trace (tests/pv_stretch_lock_reference.py) that every case
reaches the branch it names, passes the two-form gate and is well conditioned; tests/test_gpu_pv_stretch_lock_edges.py compares the kernel
with the definition on the same cases.  Test infrastructure only.

The signals are tests/pv_lock_edge_cases.py's bursts (48 samples, amp 0.6^n cos(2 pi b n / 1024), digital zero elsewhere).  Here the caller
chooses where every frame is read, so the parent's rule on the burst's start is replaced by one on the clamped positions: for every frame
f and every burst, the burst lies wholly inside [q_f, q_f + F) or wholly outside it (burst_input asserts it) -- a cut burst has a near-flat
spectrum whose peaks are decided by rounding.

A case is a name, hop, nF, n_in, bursts (start, b, amp), a position row (values below 0 and above n_in - F included), ratios (some outside
the clamp) and `expect`: (predicate, argument) pairs; a predicate counts the frames of the case's trace that take the branch (PREDICATES),
and a case that does not reach every branch it names fails the CPU file."""
from collections import namedtuple

import numpy as np

import pv_lock_cases as LC
import pv_lock_edge_cases as E
import pv_stretch_lock_reference as SLR
import pv_stretch_reference as SR

F, N_BINS = LC.F, LC.F // 2
BURST_LEN = E.BURST_LEN
StretchEdgeCase = namedtuple("StretchEdgeCase", "name hop nF n_in bursts pos ratios expect")


# ---- signals ----------------------------------------------------------------------------------------------------------------------------------
def burst_input(c):
    """float32 [n_in]: the sum of the case's bursts; every burst lies whole inside or whole outside every frame of the position row."""
    q = SR.clamp_positions(c.pos, c.n_in, F)
    x = np.zeros(c.n_in)
    n = np.arange(BURST_LEN)
    for start, b, amp in c.bursts:
        assert 0 <= start and start + BURST_LEN <= c.n_in, (c.name, start)
        for f, a in enumerate(q):
            inside = a <= start and start + BURST_LEN <= a + F
            outside = start + BURST_LEN <= a or a + F <= start
            assert inside or outside, (c.name, f, int(a), start)
        x[start:start + BURST_LEN] += amp * 0.6 ** n * np.cos(2.0 * np.pi * b * n / F)
    return x.astype(np.float32)


def length(c):
    return LC.length(c.nF, c.hop, 3)


def case_ratios(c):
    """float64 [nF], unclamped."""
    r = np.asarray(c.ratios, np.float64)
    return np.full(c.nF, float(r)) if r.ndim == 0 else r


def case_positions(c):
    return np.asarray(c.pos, np.int64)


# ---- predicates: (case, trace, argument) -> the number of frames that take the branch ------------------------------------------------------------
_count, _sounding, _has_sound = E._count, E._sounding, E._has_sound


def _step(tr, f):
    """The raw step q_f - q_(f-1) of the clamped positions (f >= 1)."""
    return tr[f]["q"] - tr[f - 1]["q"]


def _behind_silent(tr, f):
    return f > 0 and _sounding(tr[f]) and tr[f - 1]["silent"]


def p_last_silent(c, tr, m):
    return int(len(tr) % 4 == m and tr[-1]["silent"] and _has_sound(tr))


def p_silent_first(c, tr, _):
    return int(tr[0]["silent"] and _has_sound(tr))


def p_silent_slot3_late(c, tr, _):
    """A silent frame in a round's last slot, in a round behind the first, between sounding frames, the frame a round before it sounding:
    the previous phases the next round starts from were a sounding frame's until this frame handed its own down.  (In the first round
    they are the zeros of the start, which are a silent frame's phases too: a hand-over that is skipped there changes nothing.)"""
    return _count(tr, lambda f, t: t["silent"] and f % 4 == 3 and f >= 7 and f + 1 < len(tr) and _sounding(tr[f - 4]) and _sounding(tr[f + 1]))


def p_behind_silent(c, tr, kind):
    cond = {"one": lambda f, t: t["D"] == 1, "F": lambda f, t: _step(tr, f) == F, "above": lambda f, t: _step(tr, f) > F,
            "odd": lambda f, t: t["D"] % 2 == 1 and 1 < t["D"] < F, "1000": lambda f, t: t["D"] == 1000}[kind]
    return _count(tr, lambda f, t: _behind_silent(tr, f) and cond(f, t))


def p_silent_by(c, tr, kind):
    pos = case_positions(c) if c is not None else None
    cond = {"leap": lambda f: _step(tr, f) > F, "freeze": lambda f: _step(tr, f) == 0, "reverse": lambda f: _step(tr, f) < 0,
            "clamp_low": lambda f: pos[f] < 0, "clamp_high": lambda f: pos[f] > c.n_in - F}[kind]
    return _count(tr, lambda f, t: t["silent"] and (f > 0 or kind.startswith("clamp")) and cond(f)) if _has_sound(tr) else 0


def p_gone_raw(c, tr, which):
    """Every peak past N at a raw ratio of exactly 2 ("exact") or one the clamp brings to 2 ("clamped"), at an advance other than hop."""
    raw = case_ratios(c)
    return _count(tr, lambda f, t: t["gone"] and t["D"] != c.hop and ((raw[f] == 2.0) if which == "exact" else (raw[f] > 2.0)))


def p_turn_sign(c, tr, sign):
    """Sounding frames whose rotation factor (r hop - D) / F has this sign; the exact zero counts at D != hop only."""
    return _count(tr, lambda f, t: _sounding(t) and np.sign(t["r"] * c.hop - t["D"]) == sign and (sign != 0 or t["D"] != c.hop))


def p_tie_n_same_sign(c, tr, _):
    """Bin N a peak whose phase equals the previous sounding frame's, an odd D: d is exactly -1/2 with no sign flip; the ratio keeps bin N
    in band and r hop / D is no integer, so the two roundings of the half give different angles."""
    def cond(f, t):
        if not (f > 0 and not tr[f - 1]["silent"] and N_BINS in t["tie"] and t["D"] % 2 == 1 and t["r"] <= 1.0):
            return False
        return (t["r"] * c.hop / t["D"]) % 1.0 != 0.0
    return _count(tr, cond)


def p_flip_at(c, tr, k):
    """The parent's half-turn flip between two sounding frames: at bin 0 at an advance other than hop, at bin N at an even advance (an odd
    one puts the nominal term on the half turn, and the tie then needs equal signs: p_tie_n_same_sign)."""
    ok = (lambda t: t["D"] != c.hop) if k == 0 else (lambda t: t["D"] % 2 == 0)
    return _count(tr, lambda f, t: f > 0 and not tr[f - 1]["silent"] and k in t["tie"] and ok(t))


def p_mixed_align(c, tr, _):
    """Rounds of four frames that hold a sounding frame at an odd position and one at an even position."""
    n = 0
    for a in range(0, len(tr), 4):
        par = {t["q"] % 2 for t in tr[a:a + 4] if _sounding(t)}
        n += par == {0, 1}
    return n


def _off_grid(c, t):
    return len(t["P"]) > 0 and t["D"] != c.hop


def p_n_and_n1(c, tr, _):
    on = lambda k: _count(tr, lambda f, t: _off_grid(c, t) and k in E._shifted(t))                                 # noqa: E731
    return min(on(N_BINS), on(N_BINS + 1))


def p_src_below(c, tr, _):
    return _count(tr, lambda f, t: _off_grid(c, t) and t["owns"] is not None and t["r"] > 1.0 and E._src(t).min() < 0)


def p_src_above(c, tr, _):
    return _count(tr, lambda f, t: _off_grid(c, t) and t["owns"] is not None and t["r"] < 1.0 and E._src(t).max() > N_BINS)


def p_behind_silent_any(c, tr, _):
    return _count(tr, lambda f, t: _behind_silent(tr, f))


def p_single_peak(c, tr, _):
    return _count(tr, lambda f, t: len(t["P"]) == 1)


PREDICATES = {
    "silent_at": E.p_silent_at, "silent_slot3_late": p_silent_slot3_late, "last_silent": p_last_silent, "silent_rounds": E.p_silent_rounds, "silent_first": p_silent_first,
    "behind_silent": p_behind_silent, "silent_by": p_silent_by, "gone_raw": p_gone_raw, "gone_then_used": E.p_gone_then_used,
    "turn_sign": p_turn_sign, "tie_n_same_sign": p_tie_n_same_sign, "flip_at": p_flip_at, "mixed_align": p_mixed_align,
    "n_and_n1": p_n_and_n1, "src_below": p_src_below, "src_above": p_src_above,
    "any_silent": E.p_any_silent, "any_gone": E.p_any_gone, "behind_silent_any": p_behind_silent_any, "single_peak": p_single_peak,
}

# what the cases together must reach (the issue's list), each by at least one frame of a case that names it, passes gate and conditioning
REQUIRED = (
    ("silent_at", 0), ("silent_at", 1), ("silent_at", 2), ("silent_at", 3), ("silent_slot3_late", None),
    ("last_silent", 1), ("last_silent", 2), ("last_silent", 3), ("silent_rounds", None), ("silent_first", None),
    ("behind_silent", "one"), ("behind_silent", "F"), ("behind_silent", "above"), ("behind_silent", "odd"), ("behind_silent", "1000"),
    ("silent_by", "leap"), ("silent_by", "freeze"), ("silent_by", "reverse"), ("silent_by", "clamp_low"), ("silent_by", "clamp_high"),
    ("gone_raw", "exact"), ("gone_raw", "clamped"), ("gone_then_used", None),
    ("turn_sign", -1), ("turn_sign", 1), ("turn_sign", 0),
    ("tie_n_same_sign", None), ("flip_at", 0), ("flip_at", N_BINS), ("mixed_align", None),
    ("n_and_n1", None), ("src_below", None), ("src_above", None),
)

# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------
# The inputs keep their bursts on four islands, more than a frame apart, so that a position sees one whole burst or none:
#   island j starts at ISLAND[j]; a frame at ISLAND[j] - d sees it d samples behind its first sample (0 <= d <= F - 48);
#   positions in SILENT[j] see nothing.  n_in is 9001 or 9000: the last position is 7977 or 7976, silent.
ISLAND = (600, 3000, 5400, 7800)
N_IN_ODD, N_IN_EVEN = 9001, 9000
MINUS5 = LC.ratio_of(-5.0)


def _cases():
    out = []

    def add(name, hop, nF, n_in, bursts, pos, ratios, expect):
        bursts = tuple((int(p), float(b), float(a)) for p, b, a in bursts)
        assert all(e[0] in PREDICATES for e in expect) and len(pos) == nF, name
        out.append(StretchEdgeCase(name, hop, nF, n_in, bursts, tuple(int(v) for v in pos),
                                   ratios if np.ndim(ratios) == 0 else tuple(float(v) for v in ratios), tuple(expect)))

    A, B, C, D = ISLAND
    for hop in (64, 512):
        two = [(A, 100.3, 0.5), (B, 301.7, 0.4)]
        three = two + [(C, 200.4, 0.5)]
        # a silent frame at every wavefront slot, reached by a leap, a freeze, a reverse step or a clamped position; the sounding frame
        # behind it at D = 1 (a reverse step), D = F exactly, D clamped from above F, an odd D, D = 1000
        add(f"slot1-leap-one-hop{hop}", hop, 7, N_IN_ODD, two, [A - 500, 1500, A - 400, A - 340, B - 600, B - 599, B - 536], MINUS5,
            [("silent_at", 1), ("silent_by", "leap"), ("behind_silent", "one")])
        add(f"slot2-freeze-F-hop{hop}", hop, 7, N_IN_ODD, two, [A - 500, 1500, 1500, 2524, 2588, 2650, 2651], MINUS5,
            [("silent_at", 1), ("silent_at", 2), ("silent_by", "freeze"), ("behind_silent", "F")])
        add(f"slot3-reverse-above-hop{hop}", hop, 7, N_IN_ODD, two, [B - 500, B - 470, B - 440, 1200, B - 300, B - 237, B - 200], MINUS5,
            [("silent_at", 3), ("silent_by", "reverse"), ("behind_silent", "above")])
        add(f"slot0-low-odd-1000-hop{hop}", hop, 7, N_IN_ODD, [(B, 301.7, 0.4), (C, 200.4, 0.5)],
            [-500, 1800, 2577, 2600, 3500, 4500, 4563], MINUS5,
            [("silent_first", None), ("silent_at", 0), ("silent_at", 1), ("silent_by", "clamp_low"), ("silent_by", "leap"),
             ("behind_silent", "odd"), ("behind_silent", "1000")])
        add(f"high-hop{hop}", hop, 6, N_IN_EVEN, three, [A - 500, 20000, C - 450, C - 385, 2 ** 31 - 1, B - 700], [0.9, 0.9, 0.6, 1.3, 1.0, 0.75],
            [("silent_by", "clamp_high"), ("silent_at", 1), ("silent_at", 0), ("behind_silent", "one")])
        # a silent last frame at nF mod 4 = 1, 2, 3; two whole silent rounds, then a sounding frame
        for nF, n_in in ((5, N_IN_ODD), (6, N_IN_EVEN), (7, N_IN_ODD)):
            pos = [A - 500 + 61 * f for f in range(nF - 1)] + [1500]
            add(f"tail-hop{hop}-nF{nF}", hop, nF, n_in, two, pos, LC.ratio_of(3.0), [("last_silent", nF % 4)])
        add(f"rounds-hop{hop}", hop, 14, N_IN_ODD, two, [A - 500, A - 436, A - 371, A - 300] + [1000 + 37 * f for f in range(8)] + [B - 500, B - 437],
            LC.ratio_of(7.0), [("silent_rounds", None), ("silent_at", 0), ("silent_at", 3), ("behind_silent", "above")])
        # the last wavefront of the SECOND round is silent: the phases it hands down replace a sounding frame's, not the zeros of the start
        add(f"slot3-round1-hop{hop}", hop, 14, N_IN_ODD, two, [A - 500 + 40 * f for f in range(7)] + [1500] + [B - 500 + 37 * f for f in range(6)], MINUS5,
            [("silent_at", 3), ("silent_slot3_late", None), ("behind_silent", "1000")])
        # every peak leaves past N at r = 2 and at ratios the clamp brings to 2, at D != hop; the next frame (r <= 1) continues the theta
        add(f"gone-hop{hop}", hop, 7, N_IN_ODD, [(A, 403.0, 0.5), (B, 120.4, 0.5)], [A - 500, A - 450, A - 389, B - 500, B - 450, B - 401, B - 300],
            [2.0, 2.0, 3.0, 0.5, 0.75, 1.0, 0.9], [("gone_raw", "exact"), ("gone_raw", "clamped"), ("gone_then_used", None)])
        add(f"gone-inf-hop{hop}", hop, 6, N_IN_EVEN, [(A, 380.6, 0.5), (B, 77.2, 0.5)], [A - 600, A - 599, A - 300, B - 500, B - 450, B - 449],
            [2.0, np.inf, 2.0, 1.0, 0.8, 0.5], [("gone_raw", "exact"), ("gone_raw", "clamped"), ("gone_then_used", None)])
        # the rotation factor (r hop - D) / F: exactly zero at D = 0.75 hop, then positive and negative
        z = 3 * hop // 4
        add(f"turn-hop{hop}", hop, 7, N_IN_ODD, two, [A - 550, A - 550 + z, A - 550 + z + 16, B - 900, B - 900 + z, B - 880 + z, B - 100], 0.75,
            [("turn_sign", 0), ("turn_sign", 1), ("turn_sign", -1)])
        # bin N: equal signs and an odd D (freeze and reverse rows: D floors at 1) -- the tie rint's half-to-even rule decides; and the
        # parent's flips: bin N between an even and an odd offset at an even D, bin 0 between a burst and its negative at D = F
        add(f"tieN-freeze-hop{hop}", hop, 7, N_IN_ODD, [(A, 512.0, 0.5), (B, 512.0, 0.4)], [A - 500, A - 500, A - 500, A - 520, A - 520, B - 501, B - 501],
            MINUS5, [("tie_n_same_sign", None), ("flip_at", N_BINS)])
        add(f"tieN-odd-two-hop{hop}", hop, 6, N_IN_EVEN, [(600, 512.0, 0.5), (1701, 512.0, 0.4)], [500, 901, 500, 901, 902, 903], MINUS5,
            [("tie_n_same_sign", None)])
        add(f"flip0-hop{hop}", hop, 7, N_IN_ODD, [(A, 0.0, 0.5), (B, 0.0, -0.5)], [A - 500, A - 470, B - 500, B - 460, A - 400, A - 399, B - 300], 0.75,
            [("flip_at", 0)])
        # odd and even positions in one round, bursts in both
        add(f"mixed-hop{hop}", hop, 6, N_IN_EVEN, three, [A - 500, A - 435, B - 372, B - 307, C - 600, C - 537], LC.ratio_of(4.0),
            [("mixed_align", None)])
        # P' == N (341 at 1.5) beside P' == N + 1 (342 at 1.5), sources below 0; and sources above N at r = 0.5: all at D != hop
        add(f"edge15-hop{hop}", hop, 7, N_IN_ODD, [(A, 344.25, 0.5), (B, 345.25, 0.5)], [A - 500, A - 450, A - 401, B - 500, B - 450, B - 401, B - 400], 1.5,
            [("n_and_n1", None), ("src_below", None)])
        add(f"half301-hop{hop}", hop, 6, N_IN_EVEN, [(A, 302.75, 0.5), (B, 302.75, 0.5)], [A - 500, A - 450, A - 401, B - 500, B - 450, B - 401], 0.5,
            [("src_above", None)])
    # hop 256, where the branch depends on the hop: the zero rotation factor (D = 192) and the tie rule (r hop / D)
    two = [(A, 100.3, 0.5), (B, 301.7, 0.4)]
    add("turn-hop256", 256, 7, N_IN_ODD, two, [A - 550, A - 358, A - 342, B - 900, B - 708, B - 688, B - 100], 0.75,
        [("turn_sign", 0), ("turn_sign", 1), ("turn_sign", -1)])
    add("tieN-freeze-hop256", 256, 7, N_IN_ODD, [(A, 512.0, 0.5), (B, 512.0, 0.4)], [A - 500, A - 500, A - 500, A - 520, A - 520, B - 501, B - 501], MINUS5,
        [("tie_n_same_sign", None), ("flip_at", N_BINS)])
    add("slot1-leap-one-hop256", 256, 7, N_IN_ODD, two, [A - 500, 1500, A - 400, A - 340, B - 600, B - 599, B - 536], MINUS5,
        [("silent_at", 1), ("silent_by", "leap"), ("behind_silent", "one")])
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

_REF = {}


def reference(c, form="a", mutant=None):
    """(float64 [T], trace) of the case, computed once per form and mutant (callers do not write to it); form "b" has no trace."""
    key = (c.name, form, mutant)
    if key not in _REF:
        x, pos, r, T, tr = burst_input(c), case_positions(c), case_ratios(c), length(c), []
        if form == "b":
            y = SLR.stretch_locked_roundtrip_b(x, pos, T, r, F, c.hop)
        else:
            y = SLR.stretch_locked_roundtrip(x, pos, T, r, F, c.hop, mutant, trace=tr)
        y.setflags(write=False)
        _REF[key] = (y, tr)
    return _REF[key]


# (tests/pv_lock_edge_cases.py's helper reads nothing but the trace and the hop: the copy's frames still land at f hop)
structural_zero = E.structural_zero


def count(c, pred, arg, tr=None):
    return int(PREDICATES[pred](c, reference(c)[1] if tr is None else tr, arg))


def groups():
    """{(hop, nF, n_in): [cases]}: the cases stacked into one launch of at most eight streams each."""
    out = {}
    for c in CASES:
        key = (c.hop, c.nF, c.n_in)
        while len(out.get(key, [])) >= 8:
            key = key + (0,)
        out.setdefault(key, []).append(c)
    return out


GROUPS = groups()


def group_id(key):
    return f"hop{key[0]}-nF{key[1]}-n_in{key[2]}" + "-b" * (len(key) - 3)
