// vp_track_voices.inc -- the voice stage behind vp_track_body.inc, included by vp_k_yin_track_voices and vp_k_yin_track_voices_stream
// (csrc/vp_track_voices_kernels.inc): one pitch decision becomes V in-key ratios.  The definition is tests/pv_harmkey_reference.py.  In scope: lane, s,
// tau (uniform), nf0, nf1, notesN, A.fs, the harmony table of the stream's key hf0 / hf1 (entry lane, entry 64 + lane), hOff, and VC
// (VpTrackVoices).  Leaves: vr, in lane v < V the ratio of voice v.
// Also included by the fine trackers (csrc/vp_track_fine_kernels.inc) in a block where `tau` names the REFINED period, a double: this text
// may use tau only in the voiced test `tau > 0` and as the divisor of A.fs -- an integer use of it would change meaning there.
    double vr = 1.0;
    int deg = 0;
    if (lane < VC.V) {
        const size_t at = (size_t)s * VC.V + lane;
        deg = VC.degree[at];
        deg = deg < -VP_TRACK_MAX_DEGREE ? -VP_TRACK_MAX_DEGREE : deg > VP_TRACK_MAX_DEGREE ? VP_TRACK_MAX_DEGREE : deg;
        if (VC.unvoiced) vr = trk_unvoiced(VC.unvoiced[at]);
    }
    if (tau > 0) {
        // c: the index of the entry getClosestFreq returned, by the lookup's own statements (vp_track_body.inc) on the same pitch
        const double pitch = A.fs / tau;
        const int idx = __builtin_amdgcn_readfirstlane(__popcll(__ballot(lane < notesN && nf0 < pitch)) + __popcll(__ballot(lane + 64 < notesN && nf1 < pitch)));
        int c = idx;
        if (idx > 0) {
            const int im = idx - 1;
            const double fi = idx >= 64 ? trk_readlane(nf1, idx & 63) : trk_readlane(nf0, idx & 63);
            const double fim = im >= 64 ? trk_readlane(nf1, im & 63) : trk_readlane(nf0, im & 63);
            if (!(fabs(fi - pitch) <= fabs(fim - pitch))) c = im;
        }
        // voice v's entry H[max(off + c + d, 0)]: the index is lane v's, read at a uniform lane; degree 0 reads the tracker's `closest`
        int j = hOff + c + deg;
        j = j < 0 ? 0 : j;
        double ent = 0.0;
        for (int v = 0; v < VC.V; v++) {
            const int jv = __builtin_amdgcn_readlane(j, v);
            const double e = jv >= 64 ? trk_readlane(hf1, jv & 63) : trk_readlane(hf0, jv & 63);
            if (lane == v) ent = e;
        }
        if (lane < VC.V) vr = ent / pitch;
    }
