"""The gate-edge stimuli (tests/_gate_edge.py) through the CPU oracle: every stream's ring sum at the target boundary is where the
builder says, and the oracle's gate verdict flips exactly between the thr - 1 ulp and the thr streams -- which also pins the host's
bisected threshold (vp_capi.hip gate_threshold_sum, restated in _gate_edge) to the oracle's decibel comparison at the edge."""
import numpy as np
import pytest

import _gate_edge as G

FS = 44100.0


def _geom(N=1024, fs=FS):
    from oracle import oracle_py as O
    o = O.OracleStream()
    o.prepare_to_play(fs, N)
    return o.geometry()


def _oracle_verdicts(x, N, b, **params):
    """per stream: the oracle's gate verdicts (1 = gated) of the frames that start in block b, its ring sum after block b"""
    from oracle import oracle_py as O
    res = []
    for s in range(x.shape[0]):
        o = O.OracleStream(**params)
        o.prepare_to_play(FS, N)
        io = np.empty((3, N), np.float32)
        gated = None
        for k in range(b + 1):
            io[:] = x[s, :, k * N:(k + 1) * N]
            o.process_block(io)
            if k == b:
                gated = [f["gated"] for f in o.traces()]
        res.append(gated)
    return res


def test_threshold_is_the_smallest_open_sum():
    n = _geom()["inSize"]
    thr = G.gate_threshold_sum(n)
    assert not G._gate_closed(thr, n) and G._gate_closed(G.ulp_steps(thr, -1), n)
    assert abs(thr - n * 1e-6) < 1e-12 * n                      # -60 dB: rms 1e-3
    assert G.ulp_steps(thr, 1) - thr < 1e-18


@pytest.mark.parametrize("loud", [False, True])
def test_ring_sums_and_oracle_verdict_flip_at_the_threshold(loud):
    N = 1024
    g = _geom(N)
    thr = G.gate_threshold_sum(g["inSize"])
    labels, fns = zip(*G.deltas())
    targets = [f(thr) for f in fns]
    b = 8 if loud else 4
    kw = dict(loud=[(0.05 + 0.9 * s / len(targets), 0.3 * s) for s in range(len(targets))], loud_blocks=4) if loud else {}
    x, sums = G.build(g, b + 3, b, targets, **kw)
    for s in range(len(targets)):
        ring = G.ring_after_block(x[s, 0], g, b)
        assert G.seq_sum(ring) == targets[s] == sums[s], labels[s]
    i_m1, i_0 = labels.index("thr-1ulp"), labels.index("thr")
    assert targets[i_0] == thr and targets[i_m1] == G.ulp_steps(thr, -1)
    # the oracle's verdicts: frames that start in the target block (H = 768 < N: at least one) are gated exactly below thr
    verdicts = _oracle_verdicts(x, N, b, vocBool=0)
    for s, v in enumerate(verdicts):
        assert len(v) >= 1, labels[s]
        want = 1 if targets[s] < thr else 0
        assert v == [want] * len(v), (labels[s], targets[s] - thr, v)
    assert verdicts[i_m1][0] == 1 and verdicts[i_0][0] == 0


def test_synth_gate_variant_puts_the_synth_ring_at_the_threshold():
    """channel 1 (the synth ring's channel 0: the vocoder's second gate, oracle rmsSynthDb) at the edge, the voice loud"""
    N = 1024
    g = _geom(N)
    thr = G.gate_threshold_sum(g["inSize"])
    targets = [G.ulp_steps(thr, -1), thr]
    x, _ = G.build(g, 7, 4, targets, channel=1)
    for s, t in enumerate(targets):
        assert G.seq_sum(G.ring_after_block(x[s, 1], g, 4)) == t
        assert G.seq_sum(G.ring_after_block(x[s, 0], g, 4)) > 100 * thr
