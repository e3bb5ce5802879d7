"""The definition of the streaming pitch tracker (include/vp_amd.h vp_pv_tracker_*, kernels vp_k_yin_track_stream and vp_k_track_follow),
written with the batch tracker's definition tests/pv_track_reference.py.  Test infrastructure only.

A tracker of S streams, block size N >= 1, sample rate fs (8000 <= fs <= 51200) and analysis length F (1024 or 2048):
tauMax = ceil(fs / 100), W = F + tauMax.  Per stream, x is everything received since create or the stream's last reset; global block b
ends at n_b = (b + 1) N samples.

  raw decision   n_b < W: period 0, raw ratio 1.0 -- no zero-padded window is analysed.  Otherwise period and raw ratio are what
                 pv_track_reference.track(x[None, n_b - W:n_b], fs, F, F, [key]) gives for its only frame: the batch definition, same numbers
                 and operation order, on the last W samples.  Causal, no latency: block b's decision uses audio up to that block's end;
  follow stage   per stream (tgt = 1.0, age = 0, cur = 1.0); per tracker hold_blocks H (0 <= H <= 2^20) and glide g (0 < g <= 1), per block:
                     period > 0: tgt = raw ratio, age = 0;  else: age = min(age + 1, INT_MAX), tgt = 1.0 once age > H;
                     cur = tgt if g == 1.0 else cur + g * (tgt - cur)    (double; product and add are separate operations);
                     ratio[b][s] = cur.
                 H = 0 and g = 1 give the raw ratio;
  reset          a reset stream is a fresh tracker's stream: no history, follow state (1.0, 0, 1.0); H and g are the tracker's and stay.

How blocks are grouped into process() calls does not enter: the tables are a function of the blocks received.  Float32-denormal input
samples are outside the domain, as for the batch tracker.

MUTANTS are seeded faults of this definition (tests/test_pv_track_stream_reference_cpu.py requires each to differ from it on a named case).
GATHER_MUTANTS are faults of how the device collects a window from the call's slab and the stream's ring, stated on this definition's sample
indices (tests/test_pv_track_edges_cpu.py requires each to differ on a named case of tests/pv_track_edge_cases.py).  With c0 the stream's
sample count when the call began, window sample p is the stream's sample i = n_b - W + p: from the ring when i < c0, else sample j = i - c0 of
the call's slab.
  ring_phase   a sample from the ring is read one slot late: i + 1, and behind the ring's newest sample its oldest, c0 - W (0.0 where the
               ring has not been written yet);
  carry_gt     the lanes step 64 samples at a time with the offset in its block carried as (q64, r64) = (64 / N, 64 % N); the carry taken
               at `off > N` instead of `off >= N` leaves a sample that starts a block (j % N == 0, p >= 64, r64 > 0) in the block before
               it at its last offset: sample i - 1, and for j == 0 the ring's slot of i, which holds i - W."""
import numpy as np

import pv_track_reference as R

INT_MAX = 2 ** 31 - 1
HOLD_MAX = 1 << 20
GATHER_MUTANTS = ("ring_phase", "carry_gt")
MUTANTS = ("zero_prefill", "window_at_block_start", "age_ge_hold", "glide_formula_at_one", "key_ignored") + GATHER_MUTANTS


def window_len(fs, F):
    return F + R.tau_max(fs)


def follow_step(state, period, raw, hold, glide, mutant=None):
    """One block of the follow stage: state (tgt, age, cur) -> (new state, followed ratio).  Python floats are IEEE doubles and
    `cur + glide * (tgt - cur)` evaluates as a rounded difference, a rounded product and a rounded sum."""
    tgt, age, cur = state
    if period > 0:
        tgt, age = float(raw), 0
    else:
        age = min(age + 1, INT_MAX)
        if (age >= hold) if mutant == "age_ge_hold" else (age > hold):
            tgt = 1.0
    if glide == 1.0 and mutant != "glide_formula_at_one":
        cur = tgt
    else:
        step = glide * (tgt - cur)
        cur = cur + step
    return (tgt, age, cur), cur


def follow(period, raw, hold, glide, state=(1.0, 0, 1.0), mutant=None):
    """The follow stage along one stream's raw tables [n] -> (followed ratio float64 [n], final state)."""
    out = np.empty(len(period), np.float64)
    for b in range(len(period)):
        state, out[b] = follow_step(state, int(period[b]), float(raw[b]), hold, glide, mutant)
    return out, state


class StreamTracker:
    def __init__(self, S, N, fs, F, hold=0, glide=1.0, mutant=None):
        assert mutant is None or mutant in MUTANTS, mutant
        assert S >= 1 and N >= 1 and F in (1024, 2048) and R.FS_MIN <= fs <= R.FS_MAX, (S, N, fs, F)
        self.S, self.N, self.fs, self.F, self.W, self.mutant = S, N, float(fs), F, window_len(fs, F), mutant
        self.set_follow(hold, glide)
        self.reset()

    def set_follow(self, hold, glide):
        assert int(hold) == hold and 0 <= hold <= HOLD_MAX and 0.0 < glide <= 1.0, (hold, glide)
        self.hold, self.glide = int(hold), float(glide)

    def reset(self, stream=-1):
        if stream < 0:
            self.hist = [np.zeros(0, np.float32) for _ in range(self.S)]      # the stream's last samples (W + N of them at most)
            self.all = [np.zeros(0, np.float32) for _ in range(self.S)]       # ... and all of them, for the gather faults
            self.call0 = [0] * self.S                                         # the stream's count when the current call began
            self.count = [0] * self.S
            self.state = [(1.0, 0, 1.0)] * self.S
        else:
            self.hist[stream], self.count[stream], self.state[stream] = np.zeros(0, np.float32), 0, (1.0, 0, 1.0)
            self.all[stream], self.call0[stream] = np.zeros(0, np.float32), 0

    def _raw(self, s, key):
        """(period, raw ratio) of the block that just ended on stream s."""
        W, N, n, h = self.W, self.N, self.count[s], self.hist[s]
        if self.mutant == "window_at_block_start":
            if n - N < W:
                return 0, 1.0
            w = h[len(h) - N - W:len(h) - N]
        elif n < W:
            if self.mutant != "zero_prefill":
                return 0, 1.0
            w = np.concatenate([np.zeros(W - n, np.float32), h])
        elif self.mutant in GATHER_MUTANTS:
            w = self._gather_fault(s)
        else:
            w = h[len(h) - W:]
        p, r = R.track(w[None, :], self.fs, self.F, self.F, [key], mutant="key_ignored" if self.mutant == "key_ignored" else None)
        assert p.shape == (1, 1)
        return int(p[0, 0]), float(r[0, 0])

    def _gather_fault(self, s):
        W, N, n, c0, x = self.W, self.N, self.count[s], self.call0[s], self.all[s]
        at = lambda i: x[i] if i >= 0 else np.float32(0.0)                         # noqa: E731
        w = x[n - W:n].copy()
        for p in range(W):
            i = n - W + p
            if self.mutant == "ring_phase" and i < c0:
                w[p] = at(i + 1 if i + 1 < c0 else c0 - W)
            if self.mutant == "carry_gt" and p >= 64 and 64 % N and i >= c0 and (i - c0) % N == 0:
                w[p] = at(i - 1 if i > c0 else i - W)
        return w

    def process(self, blocks, keys=None):
        """blocks float32 [n][S][N] -> (period int32 [n][S], followed ratio float64 [n][S]); self.raw is the raw ratio table of the call."""
        blocks = np.asarray(blocks)
        assert blocks.dtype == np.float32 and blocks.ndim == 3 and blocks.shape[1:] == (self.S, self.N), (blocks.dtype, blocks.shape)
        if keys is None:
            keys = [12] * self.S
        elif np.ndim(keys) == 0:
            keys = [int(keys)] * self.S
        assert len(keys) == self.S
        n = blocks.shape[0]
        self.call0 = list(self.count)
        period, ratio, self.raw = np.zeros((n, self.S), np.int32), np.ones((n, self.S), np.float64), np.ones((n, self.S), np.float64)
        for b in range(n):
            for s in range(self.S):
                self.hist[s] = np.concatenate([self.hist[s], blocks[b, s]])[-(self.W + self.N):]
                if self.mutant in GATHER_MUTANTS:
                    self.all[s] = np.concatenate([self.all[s], blocks[b, s]])
                self.count[s] += self.N
                period[b, s], self.raw[b, s] = self._raw(s, keys[s])
                self.state[s], ratio[b, s] = follow_step(self.state[s], period[b, s], self.raw[b, s], self.hold, self.glide, self.mutant)
        return period, ratio


def run(blocks, fs, F, keys=None, hold=0, glide=1.0, groups=None, mutant=None):
    """The tables of a whole slab [n][S][N] from a fresh tracker, fed in calls of `groups` blocks (default: one call)."""
    n, S, N = blocks.shape
    t = StreamTracker(S, N, fs, F, hold, glide, mutant)
    ps, rs, b = [], [], 0
    for k in (groups or [n]):
        p, r = t.process(blocks[b:b + k], keys)
        ps.append(p)
        rs.append(r)
        b += k
    assert b == n
    return np.concatenate(ps), np.concatenate(rs)
