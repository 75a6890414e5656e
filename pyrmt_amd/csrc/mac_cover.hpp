// mac_cover.hpp -- where the config-5 MAC loop (mac.hip) works for one disc in box mode, as
// pure host arithmetic on a support box: plain C++, no HIP, so tools/mac_cover_check.hip runs
// it on the host against its Python restatement (tests/test_mac_geometry_cpu.py).
#pragma once
#include <algorithm>

namespace rmt {

struct MacCover {
    int cb[4];          // the cells {j0, j1, i0, i1} (half-open) this disc's passes cover
    int none_rows[2];   // the rows the no-op test scans, and
    int none_cols[2];   // the 64-column words of those rows (ExtrapCall::none_rows / none_cols)
    bool empty;         // the map holds no nonzero cell
};

// box = {j0, j1, i0, i1} (inclusive; j1 < j0: empty), the support of a disc's map
// (k_box_reduce); G: the growth in cells, layers + 6
inline MacCover mac_cover(const int box[4], int N, int G) {
    MacCover C{{0, 0, 0, 0}, {0, 1}, {0, 1}, box[1] < box[0]};
    if (C.empty) return C;   // (one row, one word: no candidate)
    int *cb = C.cb;
    cb[0] = std::max(0, box[0] - G); cb[1] = std::min(N, box[1] + 1 + G);
    cb[2] = std::max(0, box[2] - G); cb[3] = std::min(N, box[3] + 1 + G);
    // whole SL tiles: the phi pass covers exactly the cells they advected
    cb[0] -= cb[0] % 4; cb[1] = std::min(N, (cb[1] + 3) / 4 * 4);
    cb[2] -= cb[2] % 64; cb[3] = std::min(N, (cb[3] + 63) / 64 * 64);
    // the known cells lie in rows [cb0, cb1) (the known plane is cleared elsewhere), so a
    // candidate -- an unknown 8-neighbour of a known cell -- in [cb0 - 1, cb1 + 1)
    C.none_rows[0] = std::max(0, cb[0] - 1);
    C.none_rows[1] = std::min(N, cb[1] + 1);
    // likewise the columns [cb2 - 1, cb3 + 1): their 64-column words
    C.none_cols[0] = std::max(0, cb[2] - 1) >> 6;
    C.none_cols[1] = (std::min(N - 1, cb[3]) >> 6) + 1;
    return C;
}

// The rows [rows[0], rows[1]) holding every disc's covered cells, which k_mac_diag visits:
// the hull of the n non-empty cb (n = 0, boxes off: every row; every cb empty: {N, 0})
inline void mac_diag_rows(const int cb[][4], int n, int N, int rows[2]) {
    rows[0] = 0; rows[1] = N;
    if (!n) return;
    rows[0] = N; rows[1] = 0;
    for (int k = 0; k < n; ++k)
        if (cb[k][1] > cb[k][0]) {
            rows[0] = std::min(rows[0], cb[k][0]); rows[1] = std::max(rows[1], cb[k][1]);
        }
}

}  // namespace rmt
