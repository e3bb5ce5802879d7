// pv_transient_host_check.cpp -- the transient-preserving stretch's host half as a stand-alone program, for the sanitizers:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include -I vocoderproject_amd/csrc \
//         tools/pv_transient_host_check.cpp -o host_check
//
// It compiles csrc/vp_onset_host.inc -- the very text vp_capi.hip includes -- and calls vp_stretch_positions_transient and vp_onset_pick on
// the cases it reads from standard input, with every table in a heap block of exactly its size, so a write or read one element outside
// is the address sanitizer's to report.  One line in, one line out:
//     <n_frames> <hop> <stretch> <n_in> <K> <onsets as a string of 0 and 1>      ->  <rc> <pos ...> | <reset ...>
//     pick <thr> <flux ...> <mass ...>                                           ->  <rc> <onsets ...>
// tests/test_pv_transient_reference_cpu.py feeds it the sweep it also runs through the library and compares the lines with NumPy's.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "vp_onset_host.inc"

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        if (line.compare(0, 5, "pick ") == 0) {
            std::string word;
            double thr;
            in >> word >> thr;
            std::vector<double> v;
            for (double d; in >> d;) v.push_back(d);
            const int n = (int)(v.size() / 2);
            double *flux = new double[n], *mass = new double[n];
            unsigned char *on = new unsigned char[n];
            for (int i = 0; i < n; i++) { flux[i] = v[i]; mass[i] = v[n + i]; }
            std::printf("%d", vp_onset_pick(flux, mass, n, thr, on));
            for (int i = 0; i < n; i++) std::printf(" %d", on[i]);
            std::printf("\n");
            delete[] flux; delete[] mass; delete[] on;
            continue;
        }
        int nF, hop, nIn, K;
        double stretch;
        std::string bits;
        in >> nF >> hop >> stretch >> nIn >> K >> bits;
        const int nG = vp_onset_num_frames(nIn, 1024, hop);
        if (nG < 0 || (int)bits.size() != nG) { std::printf("bad line\n"); return 2; }
        unsigned char *on = new unsigned char[nG];
        for (int g = 0; g < nG; g++) on[g] = bits[g] == '1' ? 0x80 : 0;
        int *pos = new int[nF];
        unsigned char *reset = new unsigned char[nF];
        std::printf("%d", vp_stretch_positions_transient(pos, reset, nF, hop, stretch, nIn, 1024, on, K));
        for (int f = 0; f < nF; f++) std::printf(" %d", pos[f]);
        std::printf(" |");
        for (int f = 0; f < nF; f++) std::printf(" %d", reset[f]);
        std::printf("\n");
        delete[] on; delete[] pos; delete[] reset;
    }
    return 0;
}
