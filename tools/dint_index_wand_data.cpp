// dint_index_wand_data — dint_create_wand_data (the reference's `create_wand_data`, src/create_wand_data.cpp) for a caller
// that has the INDEX and not the collection: the per-list BM25 maxima come from one decode of the index on the device.
//
//   dint_index_wand_data <index_type> <index_filename> <sizes_filename> <output_filename>
//   index_type: single_rect_dint | single_packed_dint | multi_packed_dint
//   index_filename: what dint_create_freq_index wrote (dint/index_file.hpp); its header carries num_docs
//   sizes_filename: <basename>.sizes (one record: a size per document; the first num_docs are read, as dint_create_wand_data does)
//
// norm_lens come from the sizes through the host library (dinth_wand_data, no list given: the arithmetic is that call's),
// max_term_weight from dint_index_max_weights (include/dint_hip.h). The output is the version-1 wand
// file (include/dint_host.h, dinth_write_wand_data), byte for byte what dint_create_wand_data writes for the collection the
// index was built from. One stats line on stdout.
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

int main(int argc, char** argv) {
    if (argc != 5) {
        std::cerr << "Usage: " << argv[0] << " <index_type> <index_filename> <sizes_filename> <output_filename>" << std::endl;
        return 1;
    }
    try {
        const int kind = tool::kind_of_type(argv[1]);
        if (kind < 0) {
            std::cerr << "ERROR: Unknown type " << argv[1] << std::endl;
            return 1;
        }
        auto tick = std::chrono::steady_clock::now();
        tool::mapped_file m(argv[2]);
        const dint::index_file_view v = dint::view_index_file(m.data, m.bytes);
        if (int(v.header.kind) != kind) throw std::runtime_error("the index file holds another index type");
        const uint64_t num_docs = v.header.num_docs;
        const size_t n_lists = size_t(v.header.n_lists);
        tool::blob sizes;
        tool::host_ok(dinth_read_sizes(argv[3], &sizes.h), "dinth_read_sizes");
        if (sizes.size() / 4 < num_docs) throw std::runtime_error("the .sizes record is shorter than num_docs");
        std::vector<float> norm_lens(num_docs), max_term_weight(n_lists, 0.0f);
        tool::host_ok(dinth_wand_data(static_cast<const uint32_t*>(sizes.data()), num_docs, nullptr, nullptr, nullptr, 0, norm_lens.data(), nullptr),
                      "dinth_wand_data");

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
        dint_wand_data* wand = nullptr;
        dint_ok(dint_wand_data_create(0, norm_lens.data(), num_docs, &wand), "dint_wand_data_create");
        auto device_tick = std::chrono::steady_clock::now();
        dint_ok(dint_index_max_weights(qi, freqs_dict, wand, max_term_weight.data(), nullptr, nullptr), "dint_index_max_weights");
        const double device_secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - device_tick).count();
        tool::host_ok(dinth_write_wand_data(argv[4], norm_lens.data(), num_docs, max_term_weight.data(), n_lists), "dinth_write_wand_data");
        dint_wand_data_destroy(wand);
        dint_query_index_destroy(qi);
        dint_free(blocks);
        (void)hipFree(d_index);
        dint_dict_destroy(docs_dict);
        dint_dict_destroy(freqs_dict);
        const double elapsed_secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - tick).count();
        std::cout << "{\"num_docs\": " << num_docs << ", \"sequences\": " << n_lists << ", \"blocks\": " << n_blocks
                  << ", \"postings\": " << postings << ", \"max_weights_time\": " << device_secs << ", \"construction_time\": " << elapsed_secs
                  << "}" << std::endl;
    } catch (std::exception const& e) {
        std::cerr << "ERROR: " << e.what() << std::endl;
        return 1;
    }
    return 0;
}
