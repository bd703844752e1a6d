// deg_example — DegreeDistribution on the MI355X path
// (reference: src/main/java/org/apache/flink/graph/streaming/example/DegreeDistribution.java).
//
//   deg_example            the reference's built-in six events (:185-191)
//   deg_example <edges>    a file of "src trg +|-" lines (:172-182: fields split on one whitespace
//                          character, "+" = EDGE_ADDITION, anything else = EDGE_DELETION), parsed on
//                          the host; ids are dense non-negative ints
//
// Output: one "(degree,count)" line per entry of every one-event window's distribution delta: the
// degree keys whose count the event changed, with their new count, ordered by degree. These are the
// reference's records (DegreeDistributionMap, :120-131) except those for a key that an event leaves
// where it began (count[1] when one vertex leaves degree 1 and another enters it).
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

#include "gsgpu.hpp"

using namespace gelly::streaming;

int main(int argc, char** argv) {
    std::vector<int64_t> src{1, 2, 1, 2, 3, 1}, dst{2, 3, 4, 3, 4, 2};
    std::vector<uint8_t> add{1, 1, 1, 0, 1, 0};
    if (argc > 2) {
        std::cerr << "Usage: deg_example [input edges path]\n";
        return 1;
    }
    if (argc == 2) {
        src.clear();
        dst.clear();
        add.clear();
        std::ifstream in(argv[1]);
        if (!in) {
            std::cerr << "cannot open " << argv[1] << "\n";
            return 2;
        }
        std::string line;
        for (size_t ln = 0; std::getline(in, line); ++ln) {
            if (line.empty()) continue;
            std::istringstream f(line);
            long long s, t;
            std::string e;
            if (!(f >> s >> t >> e) || s < 0 || t < 0) {
                std::cerr << "line " << ln << ": expected \"src trg +|-\" with non-negative ids\n";
                return 2;
            }
            src.push_back(s);
            dst.push_back(t);
            add.push_back(e == "+" ? 1 : 0);
        }
    }
    int64_t top = 0;
    for (size_t i = 0; i < src.size(); ++i) top = std::max(top, std::max(src[i], dst[i]));
    try {
        DegreeSummary<int64_t> ds((uint64_t)top + 1);
        std::vector<uint32_t> d;
        std::vector<uint64_t> c;
        for (size_t i = 0; i < src.size(); ++i) {
            ds.foldWindow(&src[i], &dst[i], &add[i], 1);
            ds.distributionDelta(d, c);
            for (size_t k = 0; k < d.size(); ++k) std::printf("(%u,%llu)\n", d[k], (unsigned long long)c[k]);
        }
    } catch (const GsError& e) {
        std::cerr << e.what() << "\n";
        return 3;
    }
    return 0;
}
