// vp_track_fine.inc -- the sub-sample stage behind vp_track_body.inc, included by the fine trackers (csrc/vp_track_fine_kernels.inc):
// parabolic interpolation of the normalised function around the period the walk chose (step 5 of the YIN paper), then the note lookup
// again on the refined pitch.  The definition is tests/pv_track_fine_reference.py.  In scope: dn (the normalised function, still in the
// wavefront's slice: the body wrote every lag 0 .. TRK_MAXLAG and only reads behind its last barrier), tau (uniform), tauMax, lane, nf0,
// nf1, notesN, A.fs, ratio.  Leaves: tauFine (uniform; (double)tau where the rule does not refine, 0.0 unvoiced) and ratio.
    double tauFine = (double)tau;
    if (tau > 0) {
        // neither lag 0 nor the guard slot is a neighbour: the three reads lie in dn[1 .. tauMax - 1]
        if (tau - 1 >= 1 && tau + 1 <= tauMax - 1) {
            const double ya = dn[tau - 1], yb = dn[tau], yc = dn[tau + 1];
            const double den = (ya - yb) + (yc - yb);
            // (a NaN fails a comparison: the frame keeps the integer period)
            if (ya >= yb && yc >= yb && den > 0.0 && den <= 1.7976931348623157e308) tauFine = (double)tau + (0.5 * (ya - yc)) / den;
        }
        // Notes::getClosestFreq on the refined pitch, by the body's own statements
        const double pitch = A.fs / tauFine;
        const int idx = __builtin_amdgcn_readfirstlane(__popcll(__ballot(lane < notesN && nf0 < pitch)) + __popcll(__ballot(lane + 64 < notesN && nf1 < pitch)));
        const double fi = idx >= 64 ? trk_readlane(nf1, idx & 63) : trk_readlane(nf0, idx & 63);
        double closest = fi;
        if (idx > 0) {
            const int im = idx - 1;
            const double fim = im >= 64 ? trk_readlane(nf1, im & 63) : trk_readlane(nf0, im & 63);
            if (!(fabs(fi - pitch) <= fabs(fim - pitch))) closest = fim;
        }
        ratio = closest / pitch;
    }
