// vp_onset_host.inc -- the transient-preserving stretch's HOST half: onsets from the flux table, and the position table around them
// (included by vp_capi.hip; plain C++ on host arrays, no device call, so tools/pv_transient_host_check.cpp compiles the same text into a
// stand-alone program under the address and undefined-behaviour sanitizers).  The definition is tests/pv_transient_reference.py
// pick_onsets and plan_positions; both are exact (comparisons and 64-bit integers), and the library's tables equal NumPy's (tested).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "vp_amd.h"

extern "C" int vp_onset_num_frames(int n_in, int frame_len, int hop)
{
    if (frame_len <= 0 || hop <= 0 || n_in < frame_len) return VP_ERR_INVALID_ARG;
    return (n_in - frame_len) / hop + 1;
}

// frame g is an onset iff flux[g] > 0, flux[g] >= thr mass[g], flux[g] > flux[g - 1] and flux[g] >= flux[g + 1]; a missing neighbour
// counts as -inf; a NaN in a comparison makes it false
extern "C" int vp_onset_pick(const double *flux, const double *mass, int n, double thr, unsigned char *onsets)
{
    if (!flux || !mass || !onsets || n < 0 || !(thr >= 0.0 && thr <= 1.0)) return VP_ERR_INVALID_ARG;   // (a NaN fails both tests)
    for (int g = 0; g < n; g++) {
        const double v = flux[g];
        bool on = v > 0.0 && v >= thr * mass[g];
        on = on && (g == 0 || v > flux[g - 1]) && (g == n - 1 || v >= flux[g + 1]);
        onsets[g] = on ? 1 : 0;
    }
    return VP_OK;
}

extern "C" int vp_stretch_positions_transient(int *pos, unsigned char *reset, int n_frames, int hop, double stretch, int n_in, int frame_len,
                                              const unsigned char *onsets, int K)
{
    if (!pos || !reset || !onsets || n_frames < 0 || hop <= 0 || frame_len <= 0 || n_in < frame_len || !(stretch >= 0.25 && stretch <= 4.0))
        return VP_ERR_INVALID_ARG;                                             // (vp_stretch_positions's checks; a NaN fails both tests)
    if (K < VP_ONSET_SPAN_MIN || K > VP_ONSET_SPAN_MAX) return VP_ERR_INVALID_ARG;
    if (n_frames == 0) return VP_OK;
    typedef long long i64;
    const i64 nF = n_frames, nG = ((i64)n_in - frame_len) / hop + 1;
    const i64 baseLast = std::min((i64)std::floor((double)((nF - 1) * hop) / stretch), (i64)n_in - frame_len);   // vp_stretch_positions's formula
    std::memset(reset, 0, (size_t)n_frames);
    i64 f0 = 0, p0 = 0;                                                        // the last anchor
    pos[0] = 0;
    // the line from the last anchor to (f1, p1), in 64-bit integers; the anchor's own frame is already written
    const auto line = [&](i64 f1, i64 p1) {
        for (i64 f = f0 + 1; f <= f1; f++) pos[f] = (int)(p0 + ((f - f0) * (p1 - p0)) / (f1 - f0));   // (p1 >= p0: the quotient is the floor)
        f0 = f1; p0 = p1;
    };
    for (i64 g = 0; g < nG; g++) {
        if (!onsets[g]) continue;
        const i64 fc = (i64)std::floor((double)g * stretch + 0.5), a = fc - K, b = fc + K;
        const bool ok = g - K >= 0 && g + K <= nG - 1 && a > f0 && b < nF - 1 && (g - K) * hop >= p0 && (g + K) * hop <= baseLast;
        if (!ok) continue;
        line(a, (g - K) * hop);
        line(b, (g + K) * hop);
        reset[a] = 1;
    }
    if (nF - 1 > f0) line(nF - 1, baseLast);
    return VP_OK;
}
