"""The peak-locked kernels' EDGE cases (vp_k_stft_pv_lock, vp_k_pv_stream_lock of csrc/vp_stft_lock.inc): inputs that take the branches the
first matrix (tests/pv_lock_cases.py) stays away from -- frames without a peak among sounding ones, frames whose peaks all shift past
bin N, masks whose lowest (highest) set bit lies words away from bin 0 (bin N), ownership ties on a word boundary, P' == N beside
P' == N + 1, sources outside 0 .. N, the half-turn unwrap tie at bins 0 and N.  tests/test_pv_lock_edges_cpu.py asserts on the
definition's trace (tests/pv_lock_reference.py lock_stage) that every case reaches the branch it exists for, that the two forms of the
definition agree on it and that it is well conditioned; tests/test_gpu_pv_lock_edges.py compares the kernels with the definition on the
same cases.  Test infrastructure only.

The signals are short damped bursts, amp 0.6^n cos(2 pi b n / 1024) for n < 48, digital zero elsewhere: a frame that sees one whole burst
has a smooth spectrum with one peak near bin b (b = 0 and b = 512 included), two bursts in a frame give two peaks, a frame that sees none
is exactly silent.  A burst starts at most hop - 48 samples behind a multiple of the hop, so no frame ever sees part of one (frames end
at hop - 1 mod hop): a cut burst has a near-flat spectrum whose peaks are decided by rounding, which is the click plateau's condition, not
a pointwise one.

A case names its branches as `expect`: (predicate, argument) pairs; a predicate counts the frames of the case's trace that take the
branch (PREDICATES), and a case that does not reach every branch it names fails the CPU file."""
from collections import namedtuple

import numpy as np

import pv_cases
import pv_lock_cases as LC
import pv_lock_reference as LR

F, N_BINS = LC.F, LC.F // 2
BURST_LEN = 48
EdgeCase = namedtuple("EdgeCase", "name hop nF bursts ratios expect")


# ---- signals ----------------------------------------------------------------------------------------------------------------------------------
def burst_signal(T, bursts, hop):
    """float32 [T]: the sum of the bursts (start, b, amp); every burst lies whole inside T and inside every frame that sees it."""
    x = np.zeros(T)
    n = np.arange(BURST_LEN)
    for pos, b, amp in bursts:
        assert 0 <= pos and pos + BURST_LEN <= T and pos % hop <= hop - BURST_LEN, (pos, hop, T)
        x[pos:pos + BURST_LEN] += amp * 0.6 ** n * np.cos(2.0 * np.pi * b * n / F)
    return x.astype(np.float32)


def length(c):
    return LC.length(c.nF, c.hop, 3)


def case_input(c):
    return burst_signal(length(c), c.bursts, c.hop)


def case_ratios(c):
    """float64 [nF], unclamped."""
    r = np.asarray(c.ratios, np.float64)
    return np.full(c.nF, float(r)) if r.ndim == 0 else r


# ---- predicates: (case, trace, argument) -> the number of frames that take the branch ------------------------------------------------------------
def _sounding(t):
    return not t["silent"] and not t["gone"]


def _src(t):
    """Source bin of every synthesis bin of a frame with shifted peaks (may leave 0 .. N)."""
    back = np.zeros(N_BINS + 1, np.int64)
    back[t["Ps"]] = t["Pa"]
    return np.arange(N_BINS + 1) - (t["owns"] - back[t["owns"]])


def _count(tr, cond):
    return sum(1 for f, t in enumerate(tr) if cond(f, t))


def _has_sound(tr):
    return any(not t["silent"] for t in tr)


def p_silent_at(c, tr, j):
    return _count(tr, lambda f, t: t["silent"] and f % 4 == j) if _has_sound(tr) else 0


def p_last_silent(c, tr, _):
    return int(len(tr) % 4 != 0 and tr[-1]["silent"] and _has_sound(tr))


def p_silent_between(c, tr, _):
    return _count(tr, lambda f, t: t["silent"] and f % 4 in (1, 2) and f + 1 < len(tr) and not tr[f - 1]["silent"] and not tr[f + 1]["silent"])


def p_silent_rounds(c, tr, _):
    """Sounding frames directly behind two or more whole silent rounds."""
    return _count(tr, lambda f, t: not t["silent"] and f % 4 == 0 and f >= 8 and all(u["silent"] for u in tr[f - 8:f]))


def p_gone_then_used(c, tr, _):
    return _count(tr, lambda f, t: t["gone"] and f + 1 < len(tr) and _sounding(tr[f + 1]) and tr[f + 1]["r"] <= 1.0)


def p_gone_raw(c, tr, which):
    raw = case_ratios(c) if isinstance(c, EdgeCase) else None
    return _count(tr, lambda f, t: t["gone"] and ((raw[f] == 2.0) if which == "exact" else (raw[f] > 2.0)))


def p_lowest_word(c, tr, w):
    """The lowest peak lies in word w: bins 0 .. P - 1 find no set bit at or below them and walk up across w words."""
    return _count(tr, lambda f, t: len(t["P"]) and t["P"][0] // 64 == w)


def p_highest_le(c, tr, k):
    return _count(tr, lambda f, t: len(t["P"]) and t["P"][-1] <= k)


def p_single_at(c, tr, k):
    return _count(tr, lambda f, t: list(t["P"]) == [k])


def p_single_mod63(c, tr, _):
    return _count(tr, lambda f, t: len(t["P"]) == 1 and t["P"][0] % 64 == 63)


def p_half_highest_le_256(c, tr, _):
    return _count(tr, lambda f, t: t["r"] == 0.5 and len(t["Ps"]) and t["Ps"][-1] <= 256)


def p_double_lowest_ge_128(c, tr, _):
    return _count(tr, lambda f, t: t["r"] == 2.0 and len(t["Ps"]) and t["Ps"][0] >= 128)


def _mid_ties(idx):
    return [(a + b) // 2 for a, b in zip(idx[:-1], idx[1:]) if (b - a) % 2 == 0]


def p_moved_tie_across_words(c, tr, _):
    return _count(tr, lambda f, t: any((b - a) % 2 == 0 and a // 64 != b // 64 for a, b in zip(t["Ps"][:-1], t["Ps"][1:])))


def p_own_tie_at(c, tr, res):
    """Two neighbouring peaks at even distance whose middle bin has k mod 64 == res; the definition gives it to the lower."""
    def cond(f, t):
        mids = [m for m in _mid_ties(t["P"]) if m % 64 == res]
        assert all(t["own"][m] < m for m in mids)
        return bool(mids)
    return _count(tr, cond)


def p_half_integer(c, tr, _):
    return _count(tr, lambda f, t: t["r"] in (0.5, 1.5) and any(int(p) % 2 == 1 for p in t["P"]))


def _shifted(t):
    return np.floor(t["P"] * t["r"] + 0.5).astype(np.int64)


def p_lands_on(c, tr, k):
    return _count(tr, lambda f, t: len(t["P"]) and k in _shifted(t))


def p_n_and_n1(c, tr, _):
    return min(p_lands_on(c, tr, N_BINS), p_lands_on(c, tr, N_BINS + 1))


def p_src_below(c, tr, _):
    return _count(tr, lambda f, t: t["owns"] is not None and t["r"] > 1.0 and _src(t).min() < 0)


def p_src_above(c, tr, _):
    return _count(tr, lambda f, t: t["owns"] is not None and t["r"] < 1.0 and _src(t).max() > N_BINS)


def p_tie_at(c, tr, k):
    return _count(tr, lambda f, t: k in t["tie"] and f > 0 and not tr[f - 1]["silent"])


def p_any_silent(c, tr, _):
    return _count(tr, lambda f, t: t["silent"])


def p_any_gone(c, tr, _):
    return _count(tr, lambda f, t: t["gone"])


PREDICATES = {
    "silent_at": p_silent_at, "last_silent": p_last_silent, "silent_between": p_silent_between, "silent_rounds": p_silent_rounds,
    "gone_then_used": p_gone_then_used, "gone_raw": p_gone_raw, "lowest_word": p_lowest_word, "highest_le": p_highest_le,
    "single_at": p_single_at, "single_mod63": p_single_mod63, "half_highest_le_256": p_half_highest_le_256,
    "double_lowest_ge_128": p_double_lowest_ge_128, "moved_tie_across_words": p_moved_tie_across_words, "own_tie_at": p_own_tie_at,
    "half_integer": p_half_integer, "n_and_n1": p_n_and_n1, "src_below": p_src_below, "src_above": p_src_above, "tie_at": p_tie_at,
    "any_silent": p_any_silent, "any_gone": p_any_gone,
}

# what the one-shot cases together must reach (the issue's list), each by at least one frame of a case that passes gate and conditioning
REQUIRED = (
    ("silent_at", 0), ("silent_at", 1), ("silent_at", 2), ("silent_at", 3), ("last_silent", None), ("silent_between", None),
    ("silent_rounds", None), ("gone_then_used", None), ("gone_raw", "exact"), ("gone_raw", "clamped"),
    ("lowest_word", 1), ("lowest_word", 2), ("lowest_word", 8), ("highest_le", 447), ("highest_le", 0),
    ("single_at", 0), ("single_at", 512), ("single_at", 256), ("single_mod63", None),
    ("half_highest_le_256", None), ("double_lowest_ge_128", None), ("moved_tie_across_words", None),
    ("own_tie_at", 63), ("own_tie_at", 0), ("half_integer", None), ("n_and_n1", None), ("src_below", None), ("src_above", None),
    ("tie_at", 0), ("tie_at", 512),
)


# ---- one-shot cases ------------------------------------------------------------------------------------------------------------------------------
def _at(hop, f, d=0):
    """The start of a burst that frame f is the LAST to see (d samples behind frame f's first sample)."""
    return f * hop + d


def _into(hop, f, d=0):
    """The start of a burst that frame f is the FIRST to see (its last sample d samples in front of the frame's end)."""
    return f * hop + F - BURST_LEN - d


def _cases():
    out = []

    def add(name, hop, nF, bursts, ratios, expect):
        bursts = tuple((int(p), float(b), float(a)) for p, b, a in bursts)
        assert all(e[0] in PREDICATES for e in expect), name
        out.append(EdgeCase(name, hop, nF, bursts, ratios if np.ndim(ratios) == 0 else tuple(float(v) for v in ratios), tuple(expect)))

    for hop in (64, 512):
        # frame 0 alone sees the first burst; the second enters at frame `fin`: the frames between are silent
        for fin, nF in ((2, 7), (3, 7), (4, 6), (5, 14)):
            ex = [("silent_at", j) for j in range(1, fin) if j < 4] + ([("silent_at", 0)] if fin > 4 else [])
            if fin == 2:
                ex.append(("silent_between", None))
            add(f"gap-hop{hop}-in{fin}-nF{nF}", hop, nF, [(_at(hop, 0, 2), 100.3, 0.5), (_into(hop, fin, 1), 301.7, 0.4)], LC.ratio_of(-5.0), ex)
        # two whole silent rounds, then a sounding frame; and a silent last frame at nF mod 4 = 1, 2, 3
        add(f"rounds-hop{hop}", hop, 14, [(_at(hop, 1, 3), 77.2, 0.5), (_into(hop, 12), 200.4, 0.5)], LC.ratio_of(7.0),
            [("silent_rounds", None), ("silent_at", 0), ("silent_at", 3)])
    for hop, nF in ((64, 5), (512, 6), (512, 7), (128, 7)):
        add(f"tail-hop{hop}-nF{nF}", hop, nF, [(_at(hop, 1, 5), 150.6, 0.5)], LC.ratio_of(3.0), [("last_silent", None)])
    for hop in (64, 512):
        A, B = _at(hop, 1, 3), _into(hop, 2, 1)                       # A: frames 0 and 1 see it and no other; B: frame 2 is the first
        # every peak leaves past N at r = 2 (frame 0) and at a ratio the clamp brings to 2 (frame 1); frame 2 continues the advanced theta
        add(f"gone-hop{hop}", hop, 7, [(A, 403.0, 0.5), (B, 120.4, 0.5)], [2.0, 3.0, 0.5, 0.75, 1.0, 0.9, 0.8],
            [("gone_raw", "exact"), ("gone_raw", "clamped"), ("gone_then_used", None), ("any_gone", None)])
        add(f"gone512-hop{hop}", hop, 7, [(A, 512.0, 0.5), (B, 512.0, -0.4)], [1.01, np.inf, 1.0, 0.5, 0.5, 2.0, 2.0],
            [("gone_raw", "clamped"), ("gone_then_used", None), ("single_at", 512), ("lowest_word", 8), ("half_highest_le_256", None),
             ("src_above", None)])
        # one peak, at the ends of the band, in its middle and at a word's last bit; bins below (above) it walk words up (down)
        add(f"single0-hop{hop}", hop, 7, [(A, 0.0, 0.5), (B, 0.0, 0.5)], LC.ratio_of(7.0), [("single_at", 0), ("highest_le", 0)])
        add(f"single256-hop{hop}", hop, 7, [(A, 256.0, 0.5), (B, 256.0, 0.5)], [2.0, 2.0, 0.5, 2.0, 0.5, 1.5, 1.0],
            [("single_at", 256), ("lowest_word", 4), ("highest_le", 447), ("double_lowest_ge_128", None), ("half_highest_le_256", None),
             ("src_below", None), ("src_above", None)])
        add(f"single191-hop{hop}", hop, 7, [(A, 188.75, 0.5)], [2.0, 0.5, 1.0, 1.0, 1.0, 1.0, 1.0],
            [("single_at", 191), ("single_mod63", None), ("lowest_word", 2), ("double_lowest_ge_128", None), ("half_integer", None)])
        add(f"word1-hop{hop}", hop, 7, [(A, 103.0, 0.5), (B, 103.0, 0.5)], [2.0, 2.0, 2.0, 0.5, 2.0, 0.5, 2.0],
            [("lowest_word", 1), ("highest_le", 447), ("double_lowest_ge_128", None), ("src_below", None)])
        # two peaks whose middle bin is a word's last / first bit: it goes to the lower one; shifted by 0.5 the tie lies between two words
        # (at a ratio above 1, so that the middle bin is a source of the gather and its owner shows in the output; the tie63 bursts lie
        # where frames see them deep inside the window, for the tie to carry weight at hop 64)
        t63 = (63.0, 201.0) if hop == 64 else (62.75, 200.5)
        add(f"tie63-hop{hop}", hop, 7, [(B, t63[0], 0.5), (B, t63[1], 0.5)], LC.ratio_of(3.0), [("own_tie_at", 63)])
        add(f"tie0-hop{hop}", hop, 7, [(A, 60.0, 0.5), (A, 192.0, 0.5)], LC.ratio_of(4.0), [("own_tie_at", 0)])
        add(f"movedtie-hop{hop}", hop, 7, [(A, 203.0, 0.5), (A, 400.5, 0.5)], 0.5, [("moved_tie_across_words", None), ("half_highest_le_256", None)])
        # P r + 0.5 an exact integer; P' == N (341 at 1.5) and P' == N + 1 (342 at 1.5) in one case
        add(f"edge15-hop{hop}", hop, 7, [(A, 344.25, 0.5), (B, 345.25, 0.5)], 1.5, [("half_integer", None), ("n_and_n1", None), ("src_below", None)])
        add(f"half301-hop{hop}", hop, 7, [(A, 302.75, 0.5), (B, 302.75, 0.5)], 0.5, [("half_integer", None), ("src_above", None)])
        # bins 0 and N change sign between consecutive sounding frames: the unwrap sits exactly on the half turn.  That the kernels and the
        # definition resolve it alike rests on the exactly zero imaginary part that the transform of a real frame leaves in these two bins
        # (numpy's rfft, the kernels' rfft_split), not on conditioning: moved off the real axis by 1e-13 these cases move by 1e4 bounds,
        # which is why the conditioning probe of tests/test_pv_lock_edges_cpu.py moves bins 0 and N along the real axis only
        add(f"flip0-hop{hop}", hop, 7, [(A, 0.0, 0.5), (B, 0.0, -0.5)], 0.75, [("tie_at", 0)])
        add(f"flipN-even-odd-hop{hop}", hop, 7, [(A + 1, 512.0, 0.5), (B, 512.0, 0.5)], 0.75, [("tie_at", 512)])
        add(f"flipN-odd-even-hop{hop}", hop, 7, [(A, 512.0, 0.5), (B + 1, 512.0, 0.5)], 0.6, [("tie_at", 512)])
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

_REF = {}


def reference(c, form="a", mutant=None):
    """(float64 [T], trace) of the case, computed once per form and mutant (callers do not write to it); form "b" has no trace."""
    key = (c.name, form, mutant)
    if key not in _REF:
        x, r, tr = case_input(c), case_ratios(c), []
        y = LR.locked_roundtrip_b(x, r, F, c.hop) if form == "b" else LR.locked_roundtrip(x, r, F, c.hop, mutant, tr)
        y.setflags(write=False)
        _REF[key] = (y, tr)
    return _REF[key]


def structural_zero(tr, hop, T, shift=0):
    """bool [T]: output samples that no frame with a non-zero synthesis spectrum covers (its frames are silent or lost every peak past N,
    or there is none): the definition is exactly zero there by construction, not by rounding.  shift: the streaming latency."""
    z = np.ones(T, bool)
    for f, t in enumerate(tr):
        if not (t["silent"] or t["gone"]):
            z[min(T, f * hop + shift):min(T, f * hop + F + shift)] = False
    return z


def count(c, pred, arg, tr=None):
    return int(PREDICATES[pred](c, reference(c)[1] if tr is None else tr, arg))


def groups():
    """{(hop, nF): [cases]}: the one-shot cases stacked into one input of at most eight streams per launch."""
    out = {}
    for c in CASES:
        key = (c.hop, c.nF)
        while len(out.get(key, [])) >= 8:
            key = key + (0,)
        out.setdefault(key, []).append(c)
    return out


GROUPS = groups()


def group_id(key):
    return f"hop{key[0]}-nF{key[1]}" + "-b" * (len(key) - 2)


# ---- streaming -----------------------------------------------------------------------------------------------------------------------------------
# (hop, N): every stream a burst pattern and a ratio per block.  A stream is (every, first, b, amp, d, ratio pattern): bursts at samples
# 512 (first + i every) + d (alternating sign where amp < 0); block j takes pattern[j % len].
STREAM_GEOMETRIES = ((512, 17), (128, 100), (64, 256), (512, 1000))
STREAM_PATTERNS = (
    (8, 1, 100.3, 0.5, 3, (0.7, 1.3, 0.5, 2.0, 1.0)),               # sparse: mostly silent calls between sounding ones
    (1, 0, 403.0, 0.5, 2, (2.0, 2.5, 2.0)),                          # every frame loses its peak past N
    (5, 2, 512.0, 0.5, 1, (1.5, 0.5, 2.0, 0.75)),                    # bin N, sparse
    (3, 0, 256.0, 0.4, 0, (2.0, 0.5, 1.0, 1.7)),                     # P' == N at r = 2, silent every third frame at hop 512
    (7, 3, 0.0, -0.5, 4, (0.6, 1.1)),                                # bin 0, alternating sign
    (11, 4, 188.75, 0.5, 5, (2.0, 2.0, 0.5, 0.5, 1.0, 1.0, 3.0)),
)
STREAM_REQUIRED = ("first_silent", "last_silent", "all_silent_between", "all_gone", "none_after_silent", "first_silent_off0")
StreamCase = namedtuple("StreamCase", "hop N n_blocks")
STREAM_CASES = [StreamCase(hop, N, LC.stream_blocks(N)) for hop, N in STREAM_GEOMETRIES]
N_STREAMS = len(STREAM_PATTERNS)


def stream_id(c):
    return f"hop{c.hop}-N{c.N}"


def stream_input(c):
    """float32 [S][T]"""
    T = c.N * c.n_blocks
    rows = []
    for every, first, b, amp, d, _ in STREAM_PATTERNS:
        bursts, f, i = [], first, 0
        while f * 512 + d + BURST_LEN <= T:
            bursts.append((f * 512 + d, b, abs(amp) if amp > 0 or i % 2 == 0 else -abs(amp)))
            f += every
            i += 1
        rows.append(burst_signal(T, bursts, c.hop))
    return np.stack(rows)


def stream_ratios(c):
    """float64 [n_blocks][S], some outside the clamp."""
    return np.stack([[p[5][j % len(p[5])] for p in STREAM_PATTERNS] for j in range(c.n_blocks)])


def further_blocks(c):
    """Blocks of the further, sounding call behind the case's input: the burst, and two frame lengths behind it."""
    return -(-(512 + 3 * F) // c.N)


def further_input(c):
    """float32 [S][k N]: one burst per stream behind the case's input; the further call runs it at ratio FURTHER_RATIO."""
    T0, k = c.N * c.n_blocks, further_blocks(c)
    pos = (T0 // 512 + 1) * 512 + 3
    return np.stack([burst_signal(T0 + k * c.N, [(pos, 120.4 + 40.0 * s, 0.5)], c.hop)[T0:] for s in range(N_STREAMS)])


FURTHER_RATIO = 0.8


def stream_spans(c):
    return pv_cases.call_spans(c.n_blocks, LC.STREAM_CALLS)


_SREF = {}


def stream_reference(c, further=False):
    """(float64 [S][T] by LockStreamRef under the case's call spans, [S] traces, [(fa, fb)] per call): computed once.  further: with the
    further call behind it, [S][T + k N]."""
    if (c, further) not in _SREF:
        x, tab, spans = stream_input(c), stream_ratios(c), stream_spans(c)
        if further:
            k = further_blocks(c)
            x, tab, spans = np.concatenate([x, further_input(c)], axis=1), np.concatenate([tab, np.full((k, N_STREAMS), FURTHER_RATIO)]), spans + [k]
        ys, traces, calls = [], [], None
        for s in range(N_STREAMS):
            tr = []
            r = LR.LockStreamRef(c.N, c.hop, trace=tr)
            out, b0, cl = [], 0, []
            for k in spans:
                for b in range(b0, b0 + k):                              # (block by block: a frame takes the ratio of the block that completes it)
                    fa = r.nf
                    out.append(r.process(x[s, b * c.N:(b + 1) * c.N], tab[b, s]))
                    cl.append((fa, r.nf))
                b0 += k
            per_call, b0 = [], 0
            for k in spans:
                per_call.append((cl[b0][0], cl[b0 + k - 1][1]))
                b0 += k
            calls = per_call
            y = np.concatenate(out)
            y.setflags(write=False)
            ys.append(y)
            traces.append(tr)
        _SREF[c, further] = (np.stack(ys), traces, calls)
    return _SREF[c, further]


def stream_counts(c):
    """{predicate: the number of (stream, call) pairs of the case that take the branch} on LockStreamRef's bookkeeping and the trace."""
    _, traces, calls = stream_reference(c)
    n = dict.fromkeys(STREAM_REQUIRED, 0)
    for tr in traces:
        sil = [t["silent"] for t in tr]
        for i, (fa, fb) in enumerate(calls):
            if fb > fa:
                n["first_silent"] += sil[fa] and not all(sil)
                n["last_silent"] += sil[fb - 1] and not all(sil)
                n["all_silent_between"] += all(sil[fa:fb]) and not all(sil[:fa]) and not all(sil[fb:])
                n["all_gone"] += all(t["gone"] for t in tr[fa:fb])
                n["first_silent_off0"] += sil[fa] and fa % 4 != 0 and not all(sil)
            else:
                n["none_after_silent"] += fa > 0 and sil[fa - 1] and not all(sil)
    return {k: int(v) for k, v in n.items()}
