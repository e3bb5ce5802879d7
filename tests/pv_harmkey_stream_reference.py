"""The definition of the streaming key-aware voices (include/vp_amd.h vp_pv_tracker_process_blocks_voices_device, kernels
vp_k_yin_track_voices_stream and vp_k_track_follow_voices), written with tests/pv_track_stream_reference.py's raw decision and
tests/pv_harmkey_reference.py's voice stage.  Test infrastructure only.

  raw decision   tests/pv_track_stream_reference.py's: the same window, n_b < W gives period 0;
  voice stage    pv_harmkey_reference.voice_ratios on the raw period: raw[v] per voice;
  follow stage   per (stream, voice) tgt = 1.0, cur = 1.0 and ONE age = 0 per stream at the start; per block:
                     period > 0: tgt[v] = raw[v], age = 0;  else: age = min(age + 1, INT_MAX), tgt[v] = u[s][v] once age > H;
                     cur[v] = tgt[v] if g == 1.0 else cur[v] + g * (tgt[v] - cur[v])    (product and add separate);
                     ratio[b][s][v] = cur[v].
                 With d = 0 and u = 1.0 this is the mono follow stage bit for bit;
  reset          a reset stream is a fresh one: no history, every voice (1.0, 1.0), age 0;
  voices         the number of voices may differ from call to call; the voices a call does not name keep their state.

How blocks are grouped into calls changes nothing.  Output of a call: period int32 [n][S], ratio float64 [n][S][V].

MUTANTS (tests/test_pv_harmkey_reference_cpu.py requires each to differ on a named case):
  shared_target   one tgt for all voices of a stream (the last voice's);
  age_per_call    the age restarts at 0 with every call."""
import numpy as np

import pv_harmkey_reference as HR
import pv_track_stream_reference as SR

MUTANTS = ("shared_target", "age_per_call")
INT_MAX = SR.INT_MAX


class StreamVoices:
    def __init__(self, S, N, fs, F, hold=0, glide=1.0, mutant=None):
        assert mutant is None or mutant in MUTANTS, mutant
        self.raw_tracker = SR.StreamTracker(S, N, fs, F)                        # hold 0, glide 1: its ratio is the raw one; only its period is used
        self.S, self.N, self.fs, self.F, self.mutant = S, N, float(fs), F, mutant
        self.hold, self.glide = int(hold), float(glide)
        self.reset()

    def set_follow(self, hold, glide):
        assert int(hold) == hold and 0 <= hold <= SR.HOLD_MAX and 0.0 < glide <= 1.0, (hold, glide)
        self.hold, self.glide = int(hold), float(glide)

    def reset(self, stream=-1):
        self.raw_tracker.reset(stream)
        fresh = lambda: [np.ones(HR.MAX_VOICES), np.ones(HR.MAX_VOICES), 0]     # noqa: E731  (tgt, cur, age)
        if stream < 0:
            self.state = [fresh() for _ in range(self.S)]
        else:
            self.state[stream] = fresh()

    def process(self, blocks, degrees, keys=None, unvoiced=None):
        """blocks float32 [n][S][N], degrees int [V] or [S][V], unvoiced [S][V] or None -> (period [n][S], ratio [n][S][V]);
        self.raw is the call's raw table [n][S][V]."""
        blocks = np.asarray(blocks)
        n = blocks.shape[0]
        keys_, degrees, unvoiced = HR._tables(self.S, degrees, keys, unvoiced)
        V = degrees.shape[1]
        period, _ = self.raw_tracker.process(blocks, keys)
        ratio, self.raw = np.ones((n, self.S, V)), np.ones((n, self.S, V))
        for s in range(self.S):
            tgt, cur, age = self.state[s]
            if self.mutant == "age_per_call":
                age = 0
            u = [1.0] * V if unvoiced is None else [HR.sane_unvoiced(x) for x in unvoiced[s]]
            for b in range(n):
                self.raw[b, s] = HR.voice_ratios(int(period[b, s]), self.fs, keys_[s], degrees[s], None if unvoiced is None else unvoiced[s])
                if period[b, s] > 0:
                    tgt[:V] = self.raw[b, s]
                    age = 0
                else:
                    age = min(age + 1, INT_MAX)
                    if age > self.hold:
                        tgt[:V] = u
                if self.mutant == "shared_target":
                    tgt[:V] = tgt[V - 1]
                for v in range(V):
                    if self.glide == 1.0:
                        cur[v] = tgt[v]
                    else:
                        step = self.glide * (tgt[v] - cur[v])
                        cur[v] = cur[v] + step
                ratio[b, s] = cur[:V]
            self.state[s][2] = age
        return period, ratio


def run(blocks, fs, F, degrees, keys=None, unvoiced=None, hold=0, glide=1.0, groups=None, mutant=None):
    """The tables of a whole slab [n][S][N] from a fresh tracker, fed in calls of `groups` blocks (default: one call)."""
    n, S, N = blocks.shape
    t = StreamVoices(S, N, fs, F, hold, glide, mutant)
    ps, rs, b = [], [], 0
    for k in (groups or [n]):
        p, r = t.process(blocks[b:b + k], degrees, keys, unvoiced)
        ps.append(p)
        rs.append(r)
        b += k
    assert b == n
    return np.concatenate(ps), np.concatenate(rs)
