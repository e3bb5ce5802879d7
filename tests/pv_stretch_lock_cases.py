"""The locked time-stretch test matrix (vp_stft_time_stretch_locked): the items that tests/test_pv_stretch_lock_reference_cpu.py (gate,
conditioning probe, teeth, quality) and tests/test_gpu_pv_stretch_lock.py (kernel against NumPy) BOTH iterate.  Test infrastructure only.
The definition is tests/pv_stretch_lock_reference.py; signals, curves, the ripple measure, the gate tolerance and the teeth are
tests/pv_lock_cases.py's, the edge tables tests/pv_stretch_cases.py's.

An ITEM is one stream: a name, a hop, an input row, a position table, the output length and a ratio per frame.
  gate items   384: pv_lock_cases.SIGNALS x factors (0.5, 0.8, 1.37, 4.0) x curves (+7, -12, vibrato, steps) x hops (64, 256, 512), nF = 14
  edge items   144: the 1024-point pv_stretch_cases.EDGE_CASES x EDGE_ROWS (freeze, reverse, crawl, leap, ends, skew); the case's
               semitones (0 or +7) are the constant ratio
  gpu items    20 launches of five streams (every hop x nF in 1, 2, 5, 6, 19, the four curves cycled so that every hop meets each):
               streams 0-3 at floor(f hop / a), stream 4 on a seeded monotone table; an odd n_in; a tail of hop - 1 samples no frame covers
  small items  the hop-256 edge tables with n_in = F and F + 1
  big items    300 streams, five compared

Bound of the pointwise comparisons: pv_cases.bound's derivation (double transforms and stage, float32 output frames and a float32
overlap-add of O = F / hop terms), in which nothing depends on the positions or on the stage:
    |y - ref| <= 4 O 2^-24 max(1, max |ref|)       at every sample.

DEMOTED names the items that miss the conditioning probe (tests/test_pv_stretch_lock_reference_cpu.py: a spectrum moved by 1e-13 moves the
output by 1 % of the bound or more -- a peak decision or an unwrap that sits on an edge): they are held to properties only (finite and
bounded), on the CPU and on the GPU.  The conditions: at most 5 % of the named items, none at hops 64, 128 or 256.
"""
from collections import namedtuple

import numpy as np

import pv_lock_cases as LC
import pv_stretch_cases as SC
import pv_stretch_lock_reference as SLR
import pv_stretch_reference as SR

F = LC.F
GATE_TOL = LC.GATE_TOL                      # the two forms of the reference, relative to max(1, max |ref|)
TEETH = LC.TEETH                            # a mutant is at least this many GPU bounds away on a gated item chosen to see it
CONDITION_EPS, CONDITION_SEEDS, CONDITION_SHARE = 1e-13, (0, 1, 2), 0.01      # the lock family's probe
bound = LC.bound
ratio_of = LC.ratio_of
FACTORS = SC.FACTORS
HOPS = LC.GPU_HOPS

Item = namedtuple("Item", "name hop x pos T ratio")


def factor_positions(nF, hop, a):
    return np.floor(np.arange(nF, dtype=np.int64) * hop / a).astype(np.int64)


# ---- the gate matrix --------------------------------------------------------------------------------------------------------------------------
GateCase = namedtuple("GateCase", "signal factor curve hop nF")
GATE_NF = LC.GATE_NF
GATE_CASES = [GateCase(s, a, c, hop, GATE_NF) for s in LC.SIGNALS for a in FACTORS for c in LC.GATE_CURVES for hop in LC.GATE_HOPS]
assert len(GATE_CASES) == 384


def gate_id(c):
    return f"{c.signal}-x{c.factor:g}-{c.curve}-hop{c.hop}"


def gate_item(c):
    pos = factor_positions(c.nF, c.hop, c.factor)
    n_in = F + int(pos.max()) + 1
    return Item(gate_id(c), c.hop, LC.SIGNALS[c.signal](n_in, seed=c.hop), pos, LC.length(c.nF, c.hop, 3), LC.curve(c.curve, c.nF, c.hop))


# ---- the edge tables: both clamps of the advance, both clamps of the position, every alignment ----------------------------------------------------
EDGE_CASES = [c for c in SC.EDGE_CASES if c.F == F]
EdgeRow = namedtuple("EdgeRow", "case row")
EDGE_ROWS = [EdgeRow(c, s) for c in EDGE_CASES for s in range(SC.EDGE_STREAMS)]
assert len(EDGE_ROWS) == 144


def edge_id(e, n_in=None):
    c = e.case
    return f"{SC.EDGE_ROWS[e.row]}-hop{c.hop}-nF{c.nF}-{c.semitones:+g}st" + ("" if n_in is None else f"-n_in{n_in}")


def edge_item(e, n_in=None):
    c = e.case
    return Item(edge_id(e, n_in), c.hop, SC.edge_input(c, n_in)[e.row], SC.edge_positions(c, n_in)[e.row], SC.out_length(c),
                np.full(c.nF, ratio_of(c.semitones)))


def edge_case_items(c, n_in=None):
    return [edge_item(EdgeRow(c, s), n_in) for s in range(SC.EDGE_STREAMS)]


# the smallest inputs: n_in = F (every position clamps to 0) and n_in = F + 1 (positions 0 and 1 only: unaligned frames)
SMALL_CASES = [(c, F + more) for c in EDGE_CASES if c.hop == 256 for more in (0, 1)]


# ---- the GPU launches ---------------------------------------------------------------------------------------------------------------------------
GpuCase = namedtuple("GpuCase", "hop nF curve")
GPU_NF = (1, 2, 5, 6, 19)                   # every residue mod 4 of the last round, and several rounds
GPU_STREAMS = LC.GPU_STREAMS[:5]
N_STREAMS = 5
GPU_CASES = [GpuCase(hop, nF, LC.GATE_CURVES[(i * len(GPU_NF) + j) % 4]) for i, hop in enumerate(HOPS) for j, nF in enumerate(GPU_NF)]
assert all({c.curve for c in GPU_CASES if c.hop == hop} == set(LC.GATE_CURVES) for hop in HOPS)


def gpu_id(c):
    return f"hop{c.hop}-nF{c.nF}-{c.curve}"


def gpu_positions(c):
    """int64 [N_STREAMS][nF]: the four factors, then a seeded monotone table with increments in 1 .. 2 hop."""
    rows = [factor_positions(c.nF, c.hop, a) for a in FACTORS]
    steps = np.random.default_rng([c.hop, c.nF, 51]).integers(1, 2 * c.hop + 1, max(c.nF - 1, 0))
    rows.append(np.concatenate([[0], np.cumsum(steps)]).astype(np.int64))
    return np.stack(rows)


def gpu_out_length(c):
    return LC.length(c.nF, c.hop, c.hop - 1)


def gpu_in_length(c):
    n = F + int(gpu_positions(c).max()) + 1
    return n + 1 - n % 2                                                         # odd


def gpu_items(c):
    pos, n_in, T = gpu_positions(c), gpu_in_length(c), gpu_out_length(c)
    return [Item(f"{gpu_id(c)}-s{s}", c.hop, LC.SIGNALS[GPU_STREAMS[s]](n_in, seed=c.hop + c.nF), pos[s], T, LC.curve(c.curve, c.nF, c.hop, s))
            for s in range(N_STREAMS)]


# ---- more workgroups than compute units -----------------------------------------------------------------------------------------------------------
BIG_S, BIG_CHECKED = SC.BIG_S, SC.BIG_CHECKED
BIG_HOP, BIG_NF, BIG_T, BIG_N_IN = SC.BIG_HOP, SC.BIG_NF, SC.BIG_T, SC.BIG_N_IN


def big_ratios():
    """[BIG_S][BIG_NF]: every stream its own phase of the vibrato."""
    return np.stack([LC.curve("vibrato", BIG_NF, BIG_HOP, s) for s in range(BIG_S)])


def big_items():
    x, pos, r = SC.big_input(), SC.big_positions(), big_ratios()
    return [Item(f"big-s{s}", BIG_HOP, x[s], pos[s].astype(np.int64), BIG_T, r[s]) for s in BIG_CHECKED]


# ---- references, once per item ----------------------------------------------------------------------------------------------------------------------
_REF = {}


def reference(it, form="a", mutant=None):
    """float64 [T], once per item, form and mutant (callers do not write to it)."""
    key = (it.name, form, mutant)
    if key not in _REF:
        if form == "b":
            y = SLR.stretch_locked_roundtrip_b(it.x, it.pos, it.T, it.ratio, F, it.hop)
        else:
            y = SLR.stretch_locked_roundtrip(it.x, it.pos, it.T, it.ratio, F, it.hop, mutant)
        y.setflags(write=False)
        _REF[key] = y
    return _REF[key]


def gate_and_probe(it):
    """(gate, moved / bound): the two forms' difference relative to max(1, max |ref|), and the largest move of the output under the
    conditioning probe as a share of the item's GPU bound."""
    y = reference(it)
    gate = np.abs(y - reference(it, "b")).max() / max(1.0, float(np.abs(y).max()))
    moved = max(np.abs(SLR.stretch_locked_roundtrip(it.x, it.pos, it.T, it.ratio, F, it.hop, perturb=(CONDITION_EPS, s)) - y).max()
                for s in CONDITION_SEEDS)
    return gate, moved / bound(it.hop, y)


# items that miss the conditioning probe: properties only (finite and bounded), by name
# (17 of the 528 gate and edge items, 3.2 %, every one at hop 512; all of them pass the gate.  None of the GPU, small or big items.)
DEMOTED = (
    "voice-x0.8-+7-hop512", "voice-x0.8--12-hop512", "voice-x0.8-vibrato-hop512", "voice-x0.8-steps-hop512",
    "tone-x0.8--12-hop512", "tone-x0.8-vibrato-hop512", "tone-x0.8-steps-hop512",
    "tone-tone-x0.8-+7-hop512", "tone-tone-x0.8--12-hop512", "tone-tone-x0.8-steps-hop512",
    "tone-tone-x1.37-+7-hop512", "tone-tone-x1.37-vibrato-hop512",
    "tone-tone-x4-+7-hop512", "tone-tone-x4--12-hop512", "tone-tone-x4-vibrato-hop512", "tone-tone-x4-steps-hop512",
    "ends-hop512-nF6-+7st",
)


def pointwise(it):
    return it.name not in DEMOTED


def ceiling(it):
    """pv_cases.magnitude_ceiling over the frames the item analyses: |y| <= 2 Mf, Mf = 2 max_f sum_k |X_f[k]| / F, whatever the phases are
    (the stage translates and rotates bins, and drops those that leave the band)."""
    x = np.asarray(it.x, np.float64)
    w = np.sqrt(0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(F) / F))
    q = SR.clamp_positions(it.pos, len(x), F)
    return 2.0 * (2.0 * max(float(np.abs(np.fft.rfft(x[a:a + F] * w)).sum()) for a in q) / F)


# ---- teeth: mutant -> the gated item chosen to see it -----------------------------------------------------------------------------------------------
TEETH_CASES = {
    "hop": GateCase("voice", 0.5, "+7", 256, GATE_NF),           # D = 2 hop at every frame: an unwrap with hop halves every partial's frequency offset
    "nod": GateCase("voice", 1.37, "vibrato", 256, GATE_NF),     # D != hop: the rotation must take the analysis advance out
    "late": GateCase("voice", 0.8, "steps", 256, GATE_NF),
    "nohigh": EdgeRow(next(c for c in EDGE_CASES if c.hop == 256 and c.nF == 19 and c.semitones == 7.0), SC.EDGE_ROWS.index("leap")),
}


def teeth_item(mutant):
    c = TEETH_CASES[mutant]
    return edge_item(c) if isinstance(c, EdgeRow) else gate_item(c)


# ---- quality: envelope ripple of stationary tones under (stretch, shift) ------------------------------------------------------------------------------
QUALITY_TONES = LC.QUALITY_TONES
QUALITY_PAIRS = ((0.5, 0.0), (1.5, 0.0), (0.25, 0.0), (2.0, 7.0), (0.5, -5.0))      # (stretch, semitones)
QUALITY_HOP = 256
QUALITY_T = LC.QUALITY_T                    # the OUTPUT's length; the input is as long as the stretch needs


def quality_setup(freq, stretch):
    """(x float32 [n_in], pos int [nF], T): a 0.5-amplitude tone long enough for the output's frames at this stretch."""
    nF = (QUALITY_T - F) // QUALITY_HOP + 1
    n_in = F + int(np.floor((nF - 1) * QUALITY_HOP / stretch)) + 1
    x = (0.5 * np.sin(2 * np.pi * freq * np.arange(n_in) / LC.FS)).astype(np.float32)
    return x, SR.stretch_positions(nF, QUALITY_HOP, stretch, n_in, F).astype(np.int64), QUALITY_T


def peak_frequency(y):
    """The spectral maximum of the trimmed output in Hz (Hann window, parabolic interpolation of the log magnitude)."""
    a = np.asarray(y, np.float64)[LC.QUALITY_TRIM:-LC.QUALITY_TRIM]
    n = 1 << 18
    m = np.abs(np.fft.rfft(a * np.hanning(len(a)), n))
    k = int(np.argmax(m))
    la, lb, lc = np.log(m[k - 1]), np.log(m[k]), np.log(m[k + 1])
    return (k + 0.5 * (la - lc) / (la - 2 * lb + lc)) * LC.FS / n
