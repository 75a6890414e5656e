// mac_cover_check.hip -- host run of mac_cover (pyrmt_amd/csrc/mac_cover.hpp), for the test
// that holds covered() of tests/test_mac_geometry_cpu.py to it.
//
//   hipcc -O2 -std=c++17 -o mac_cover_check tools/mac_cover_check.hip
//   mac_cover_check < lines of "N G j0 j1 i0 i1"   (the box inclusive; j1 < j0: empty)
//
// Prints per line: cb0 cb1 cb2 cb3  none_rows0 none_rows1  none_cols0 none_cols1  empty
#include <cstdio>
#include "../pyrmt_amd/csrc/mac_cover.hpp"

int main() {
    int N, G, b[4];
    while (scanf("%d %d %d %d %d %d", &N, &G, &b[0], &b[1], &b[2], &b[3]) == 6) {
        const rmt::MacCover C = rmt::mac_cover(b, N, G);
        printf("%d %d %d %d %d %d %d %d %d\n", C.cb[0], C.cb[1], C.cb[2], C.cb[3], C.none_rows[0],
               C.none_rows[1], C.none_cols[0], C.none_cols[1], (int)C.empty);
    }
    return 0;
}
