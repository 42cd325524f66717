// dint_check_index — the reference's `check_index` tool (src/check_index.cpp; verify_collection, include/ds2i/verify_collection.hpp:7-52,
// also behind `create_freq_index --check`): does the index hold the collection it was built from?
//
//   dint_check_index <index_type> <index_filename> <collection_basename>
//   index_type: single_rect_dint | single_packed_dint | multi_packed_dint
//   index_filename: what dint_create_freq_index wrote (dint/index_file.hpp)
//   collection_basename: <basename>.docs / <basename>.freqs, the reference's binary_freq_collection: every sequence is
//   [n][values...], and .docs opens with the singleton [1][num_docs]
//
// The collection files are mapped and handed to dint_check_index (include/dint_hip.h) as they are: one
// walk over the length words finds where every list begins, no posting is copied. The index is decoded on the device, every
// list compared with the collection's. "Everything is OK!" on stderr and exit status 0; on a mismatch the reference's
// message for the first one (wrong length, docid, freq) and exit status 1, as its exit(1). One stats line on stdout.
#include <hip/hip_runtime.h>

#include <chrono>
#include <iostream>
#include <string>
#include <vector>

#include "dint/index_file.hpp"
#include "dint_hip.h"
#include "tool_common.hpp"

static void dint_ok(int st, const char* what) {
    if (st != DINT_OK) throw std::runtime_error(std::string(what) + ": " + dint_strerror(st) + " " + dint_last_hip_error());
}

// Where the sequences of a collection file begin (word offsets of their first values) and how long they are. The reader's
// rules (binary_collection.hpp:131-146): a record of length 0 is skipped. A record that claims more values than the file
// holds is an error here — the reference cuts it short, and an index built from the cut list would pass; a check should say.
static void walk_sequences(tool::mapped_file const& f, std::string const& name, std::vector<uint64_t>& at, std::vector<uint64_t>& len) {
    if (f.bytes % 4 != 0) throw std::runtime_error(name + " is truncated (not a whole number of words)");
    uint32_t const* w = f.words();
    const size_t size = f.n_words();
    for (size_t pos = 0; pos != size;) {
        const uint64_t n = w[pos++];
        if (n == 0) continue;
        if (n > size - pos) throw std::runtime_error(name + " is truncated (a sequence runs past the end of the file)");
        at.push_back(pos);
        len.push_back(n);
        pos += size_t(n);
    }
}

int main(int argc, char** argv) {
    if (argc != 4) {
        std::cerr << "Usage: " << argv[0] << " <index_type> <index_filename> <collection_basename>" << std::endl;
        return 1;
    }
    bool ok = false;
    try {
        const std::string type = argv[1], basename = argv[3];
        const int kind = tool::kind_of_type(type);
        if (kind < 0) {
            std::cerr << "ERROR: Unknown type " << type << std::endl;
            return 1;
        }
        tool::mapped_file m(argv[2]);
        const dint::index_file_view v = dint::view_index_file(m.data, m.bytes);
        if (int(v.header.kind) != kind) throw std::runtime_error("the index file holds another index type");
        const size_t n_lists = size_t(v.header.n_lists);

        tool::mapped_file docs(basename + ".docs"), freqs(basename + ".freqs");
        std::vector<uint64_t> docs_at, docs_len, freqs_at, freqs_len;
        walk_sequences(docs, basename + ".docs", docs_at, docs_len);
        walk_sequences(freqs, basename + ".freqs", freqs_at, freqs_len);
        // binary_freq_collection (include/ds2i/binary_freq_collection.hpp:14-23)
        if (docs_len.empty() || docs_len.front() != 1) throw std::invalid_argument("First sequence should only contain number of documents");
        docs_at.erase(docs_at.begin());
        docs_len.erase(docs_len.begin());
        if (docs_len != freqs_len) throw std::runtime_error("docs and freqs files do not match");
        if (docs_len.size() != n_lists)
            throw std::runtime_error("the collection holds " + std::to_string(docs_len.size()) + " sequences, the index " + std::to_string(n_lists));

        dint_dict *docs_dict = nullptr, *freqs_dict = nullptr;
        dint_ok(dint_dict_create(kind, v.docs_dict, size_t(v.header.docs_dict_bytes), 0, &docs_dict), "dint_dict_create(docs)");
        dint_ok(dint_dict_create(kind, v.freqs_dict, size_t(v.header.freqs_dict_bytes), 0, &freqs_dict), "dint_dict_create(freqs)");
        dint_block_ref* blocks = nullptr;
        size_t n_blocks = 0;
        uint64_t postings = 0;
        dint_ok(dint_index_posting_lists(v.index, size_t(v.header.index_bytes), v.offsets, n_lists, &blocks, &n_blocks, &postings),
                "dint_index_posting_lists");
        uint8_t* d_index = nullptr;
        const size_t index_bytes = size_t(v.header.index_bytes) + 16;  // (the kernels fetch whole words)
        if (hipMalloc(&d_index, index_bytes) != hipSuccess || hipMemset(d_index, 0, index_bytes) != hipSuccess ||
            hipMemcpy(d_index, v.index, size_t(v.header.index_bytes), hipMemcpyHostToDevice) != hipSuccess)
            throw std::runtime_error("could not place the index on the device");
        dint_query_index* qi = nullptr;
        dint_ok(dint_query_index_create(docs_dict, d_index, index_bytes, blocks, n_blocks, n_lists, &qi), "dint_query_index_create");

        dint_collection_view view{};
        view.docs = docs.words(), view.freqs = freqs.words();
        view.docs_at = docs_at.data(), view.freqs_at = freqs_at.data(), view.list_len = docs_len.data(), view.n_lists = n_lists;
        uint64_t mismatches = 0;
        dint_index_mismatch first{};
        std::cerr << "Checking the written data, just to be extra safe..." << std::endl;
        auto tick = std::chrono::steady_clock::now();
        dint_ok(dint_check_index(qi, freqs_dict, &view, &mismatches, &first, nullptr), "dint_check_index");
        const double check_secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - tick).count();
        dint_query_index_destroy(qi);
        dint_free(blocks);
        (void)hipFree(d_index);
        dint_dict_destroy(docs_dict);
        dint_dict_destroy(freqs_dict);

        // verify_collection.hpp:18-46, the reference's wording
        if (first.kind == DINT_CHECK_LENGTH) {
            std::cerr << "sequence " << first.list << " has wrong length! (" << first.got << " != " << first.expected << ")" << std::endl;
        } else if (first.kind == DINT_CHECK_DOCID || first.kind == DINT_CHECK_FREQ) {
            std::cerr << (first.kind == DINT_CHECK_DOCID ? "docid" : "freq") << " in sequence " << first.list << " differs at position "
                      << first.position << "!" << std::endl;
            std::cerr << first.got << " != " << first.expected << std::endl;
            std::cerr << "sequence length: " << docs_len[first.list] << std::endl;
        } else {
            std::cerr << "Everything is OK!" << std::endl;
        }
        ok = mismatches == 0;
        std::cout << "{\"type\": \"" << type << "\", \"sequences\": " << n_lists << ", \"postings\": " << postings
                  << ", \"mismatches\": " << mismatches;
        if (!ok) {
            static const char* const kinds[] = {"ok", "length", "docid", "freq"};
            std::cout << ", \"first\": {\"kind\": \"" << kinds[first.kind & 3] << "\", \"sequence\": " << first.list
                      << ", \"position\": " << first.position << ", \"expected\": " << first.expected << ", \"got\": " << first.got << "}";
        }
        std::cout << ", \"check_time\": " << check_secs << "}" << std::endl;
    } catch (std::exception const& e) {
        std::cerr << "ERROR: " << e.what() << std::endl;
        return 1;
    }
    return ok ? 0 : 1;
}
