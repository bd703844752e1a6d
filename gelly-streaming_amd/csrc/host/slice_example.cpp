// slice_example — SnapshotStream on the MI355X path: per-vertex sums of edge values over one window
// (reference: SimpleEdgeStream.slice(size, direction).reduceOnEdges(sum), SimpleEdgeStream.java:135-167,
// SnapshotStream.java:100-120).
//
//   slice_example [out|in|all]    the seven (src, dst, value) edges of the reference's test stream,
//                                 sliced as one window in the given direction (default out)
//
// Output: one "vertex,sum" line per vertex with an entry in the window, ordered by vertex.
#include <cstdio>
#include <iostream>
#include <string>

#include "gsgpu.hpp"

using namespace gelly::streaming;

int main(int argc, char** argv) {
    const std::vector<int64_t> src{1, 1, 2, 3, 3, 4, 5}, dst{2, 3, 3, 4, 5, 5, 1}, val{12, 13, 23, 34, 35, 45, 51};
    const std::string d = argc > 1 ? argv[1] : "out";
    if (argc > 2 || (d != "out" && d != "in" && d != "all")) {
        std::cerr << "Usage: slice_example [out|in|all]\n";
        return 1;
    }
    const uint32_t dir = d == "out" ? GS_SLICE_OUT : d == "in" ? GS_SLICE_IN : GS_SLICE_ALL;
    try {
        SnapshotStream<int64_t> ss(6, dir);
        ss.window(src.data(), dst.data(), val.data(), src.size());
        std::vector<int64_t> v, x;
        ss.reduceOnEdges(GS_SLICE_SUM, v, x);
        for (size_t k = 0; k < v.size(); ++k) std::printf("%lld,%lld\n", (long long)v[k], (long long)x[k]);
    } catch (const GsError& e) {
        std::cerr << e.what() << "\n";
        return 3;
    }
    return 0;
}
