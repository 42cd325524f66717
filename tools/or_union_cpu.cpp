// One CPU core answering or_query<false> over lists that are already decoded: the reference's loop (include/ds2i/queries.hpp:
// 86-130) — every cursor on the current docID steps, the next docID is the smallest cursor — over plain arrays, so that the
// timing holds the union alone (no decode). The CPU side of the OR timings in DESIGN.md (tests/or_query_timing.py builds
// this file into a shared object and calls it through ctypes).
//
//   g++ -O2 -shared -fPIC -o libor_union_cpu.so tools/or_union_cpu.cpp
#include <cstddef>
#include <cstdint>
#include <vector>

extern "C" uint64_t or_union_count(const uint32_t* const* lists, const uint64_t* lens, size_t k) {
    const uint64_t end = uint64_t(1) << 32;  // past every docID (num_docs of the reference's loop)
    std::vector<uint64_t> pos(k, 0);
    auto docid = [&](size_t i) { return pos[i] < lens[i] ? uint64_t(lists[i][pos[i]]) : end; };
    uint64_t cur = end;
    for (size_t i = 0; i != k; ++i)
        if (docid(i) < cur) cur = docid(i);
    uint64_t results = 0;
    while (cur < end) {
        results += 1;
        uint64_t next = end;
        for (size_t i = 0; i != k; ++i) {
            if (docid(i) == cur) pos[i] += 1;
            if (docid(i) < next) next = docid(i);
        }
        cur = next;
    }
    return results;
}
