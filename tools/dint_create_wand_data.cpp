// dint_create_wand_data — the reference's `create_wand_data` tool (src/create_wand_data.cpp, include/ds2i/wand_data.hpp:18-57).
//
//   dint_create_wand_data <collection_basename> <output_filename>
//
// Reads <basename>.sizes (one record: a size per document), <basename>.docs and <basename>.freqs, and writes the BM25
// document lengths (norm_lens) and per-list maxima (max_term_weight) that `dint_queries ... ranked_and <index> <wand_file>`
// reads. The file is this repository's own layout (include/dint_host.h, dinth_write_wand_data), not the reference's
// succinct::mapper::freeze image. One stats line on stdout.
#include <chrono>
#include <iostream>

#include "tool_common.hpp"

int main(int argc, char** argv) {
    if (argc != 3) {
        std::cerr << "Usage: " << argv[0] << " <collection basename> <output filename>" << std::endl;
        return 1;
    }
    try {
        const std::string basename = argv[1];
        auto tick = std::chrono::steady_clock::now();
        tool::mapped_file sizes(basename + ".sizes"), docs(basename + ".docs"), freqs(basename + ".freqs");
        tool::blob norm_lens, max_term_weight;
        uint64_t num_docs = 0;
        tool::host_ok(dinth_wand_data_collection(sizes.words(), sizes.n_words(), docs.words(), docs.n_words(), freqs.words(),
                                                 freqs.n_words(), &norm_lens.h, &max_term_weight.h, &num_docs),
                      "dinth_wand_data_collection");
        const uint64_t n_lists = max_term_weight.size() / 4;
        tool::host_ok(dinth_write_wand_data(argv[2], static_cast<float const*>(norm_lens.data()), num_docs,
                                            static_cast<float const*>(max_term_weight.data()), n_lists),
                      "dinth_write_wand_data");
        const double elapsed_secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - tick).count();
        std::cout << "{\"num_docs\": " << num_docs << ", \"sequences\": " << n_lists << ", \"construction_time\": " << elapsed_secs
                  << "}" << std::endl;
    } catch (std::exception const& e) {
        std::cerr << "ERROR: " << e.what() << std::endl;
        return 1;
    }
    return 0;
}
