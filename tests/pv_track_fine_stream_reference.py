"""The definition of the streaming FINE pitch tracker (include/vp_amd.h vp_pv_tracker_process_blocks_fine_device and vp_pv_tracker_set_mode,
kernels vp_k_yin_track_stream_fine and vp_k_yin_track_voices_stream_fine): tests/pv_track_stream_reference.py with the raw decision of
tests/pv_track_fine_reference.py.  Test infrastructure only.

  raw decision   n_b < W: period 0, refined period 0.0, raw ratio 1.0.  Otherwise what pv_track_fine_reference.track_fine gives for the
                 only frame of the last W samples taken as a row;
  follow stage   pv_track_stream_reference's, unchanged: it reads the period only as the voiced flag;
  period_fine    the raw decision's refined period, before the follow stage: it is not held and not glided;
  mode           a tracker switched between the integer and the fine decision keeps ring, counters and follow state: only the raw
                 decision of the blocks that follow changes (StreamTracker.fine is read per call);
  voices         pv_harmkey_stream_reference's follow stage per voice on pv_track_fine_reference.voice_ratios_fine of the refined period."""
import numpy as np

import pv_harmkey_reference as HR
import pv_harmkey_stream_reference as HSR
import pv_track_fine_reference as FR
import pv_track_stream_reference as SR


class FineStreamTracker(SR.StreamTracker):
    """SR.StreamTracker whose raw decision is the fine one while self.fine is set (the default); process() also leaves self.period_fine,
    float64 [n][S] (with self.fine unset: the integer period as a double)."""
    fine = True

    def _raw(self, s, key):
        n, h = self.count[s], self.hist[s]
        if n < self.W:
            self._log.append(0.0)
            return 0, 1.0
        if not self.fine:
            p, r = super()._raw(s, key)
            self._log.append(float(p))
            return p, r
        p, pf, r = FR.track_fine(h[len(h) - self.W:][None, :], self.fs, self.F, self.F, [key])
        self._log.append(float(pf[0, 0]))
        return int(p[0, 0]), float(r[0, 0])

    def process(self, blocks, keys=None):
        self._log = []
        period, ratio = super().process(blocks, keys)
        self.period_fine = np.asarray(self._log, np.float64).reshape(period.shape)      # (_raw runs block by block, stream by stream)
        return period, ratio


class FineStreamVoices(HSR.StreamVoices):
    """HSR.StreamVoices with the fine raw decision: the same state and follow statements, the voice stage on the refined period."""
    fine = True

    def __init__(self, S, N, fs, F, hold=0, glide=1.0):
        super().__init__(S, N, fs, F, hold, glide)
        self.raw_tracker = FineStreamTracker(S, N, fs, F)

    def process(self, blocks, degrees, keys=None, unvoiced=None):
        blocks = np.asarray(blocks)
        n = blocks.shape[0]
        keys_, degrees, unvoiced = HR._tables(self.S, degrees, keys, unvoiced)
        V = degrees.shape[1]
        self.raw_tracker.fine = self.fine
        period, _ = self.raw_tracker.process(blocks, keys)
        fine = self.raw_tracker.period_fine
        ratio, self.raw = np.ones((n, self.S, V)), np.ones((n, self.S, V))
        for s in range(self.S):
            tgt, cur, age = self.state[s]
            u = [1.0] * V if unvoiced is None else [HR.sane_unvoiced(x) for x in unvoiced[s]]
            for b in range(n):
                self.raw[b, s] = FR.voice_ratios_fine(fine[b, s], self.fs, keys_[s], degrees[s], None if unvoiced is None else unvoiced[s])
                if period[b, s] > 0:
                    tgt[:V] = self.raw[b, s]
                    age = 0
                else:
                    age = min(age + 1, HSR.INT_MAX)
                    if age > self.hold:
                        tgt[:V] = u
                for v in range(V):
                    if self.glide == 1.0:
                        cur[v] = tgt[v]
                    else:
                        step = self.glide * (tgt[v] - cur[v])
                        cur[v] = cur[v] + step
                ratio[b, s] = cur[:V]
            self.state[s][2] = age
        return period, ratio


def run(blocks, fs, F, keys=None, hold=0, glide=1.0, groups=None, fine=None):
    """(period, period_fine, followed ratio) of a whole slab [n][S][N] from a fresh tracker, fed in calls of `groups` blocks (default: one
    call); fine: per call, whether the call runs in the fine mode (default: every call)."""
    n, S, N = blocks.shape
    t = FineStreamTracker(S, N, fs, F, hold, glide)
    ps, fs_, rs, b = [], [], [], 0
    for i, k in enumerate(groups or [n]):
        t.fine = True if fine is None else bool(fine[i])
        p, r = t.process(blocks[b:b + k], keys)
        ps.append(p)
        fs_.append(t.period_fine)
        rs.append(r)
        b += k
    assert b == n
    return np.concatenate(ps), np.concatenate(fs_), np.concatenate(rs)
