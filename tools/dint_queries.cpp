// dint_queries — the reference's `queries` tool (src/queries.cpp:15-153) for the DINT index types, on the device path.
//
//   dint_queries <index_type> <query_type> <index_filename> [<wand_filename>] [--batch] [--runs R] [--filter FILE] [--facets FILE] [--pages N]
//                [--per-group N] [--values FILE] [--order asc|desc] [--value-range lo:hi] [--edges e1,e2,...] [--percentiles p1,p2,...] [--top-values N] < query_log
//   index_type: single_rect_dint | single_packed_dint | multi_packed_dint        (include/index_types.hpp:73-79)
//   query_type: and | and_freq | or | or_freq | ranked_and | ranked_or | ranked_or_maxscore | ranked_or_blockmax | ranked_bool |
//               ranked_or_bool | ranked_or_range | ranked_and_range | ranked_or_filtered | ranked_and_filtered |
//               ranked_or_faceted | ranked_and_faceted | ranked_or_collapsed | ranked_and_collapsed | ranked_or_paged |
//               ranked_and_paged | ranked_or_sorted | ranked_and_sorted | ranked_or_value_stats | ranked_and_value_stats |
//               ranked_or_group_stats | ranked_and_group_stats | ranked_or_percentiles | ranked_and_percentiles |
//               ranked_or_top_values | ranked_and_top_values |
//               ranked_or_group_limit | ranked_and_group_limit, several
//               separated by ':'
//               (src/queries.cpp:93-111);
//               ranked_and (BM25 top 10, as the reference's driver asks for) needs the wand file, and without one prints
//               "Unsupported query type", as the reference does; ranked_or (ranked_or_query, include/ds2i/queries.hpp:387-457,
//               BM25 top 10 of the union) is not in the reference driver's list, and is answered as ranked_and is, with
//               the wand file, and refused the same way without one; ranked_or_maxscore is ranked_or with MaxScore's pruning
//               (the same results; the wand file's max_term_weight goes to the device handle), also only with a wand file;
//               ranked_or_blockmax is ranked_or_maxscore on a handle that also carries block maxima, computed from the index
//               at start-up (dint_index_max_weights, dint_wand_data_set_block_max_weights);
//               ranked_bool (dint_ranked_bool_queries, BM25 top 10 of the documents that hold every required and no
//               excluded term, the optional terms counted where they occur) reads its query lines as
//               tokens — +t required, -t excluded, a bare t optional — and so must be the only type of its run; also only
//               with a wand file;
//               ranked_or_bool (dint_ranked_or_bool_queries, BM25 top 10 of the documents that hold at least m of the optional
//               and no excluded term) reads its lines as tokens too — a bare t optional, -t excluded,
//               ~m the line's minimum (at most one; without it 1) — refuses +t, and must be the only type of its run as
//               well; also only with a wand file;
//               ranked_or_range / ranked_and_range (dint_ranked_or_range_queries, dint_ranked_and_range_queries: ranked_or /
//               ranked_and over the documents of a docID interval) read their lines as term ids plus at
//               most one @lo:hi token — the line's half-open range [lo, hi); without it the line is unrestricted — and so
//               each must be the only type of its run; also only with a wand file; output and keys are ranked_or's;
//               ranked_or_filtered / ranked_and_filtered (dint_ranked_or_filtered_queries, dint_ranked_and_filtered_queries:
//               ranked_or / ranked_and over the documents of one filter for the whole log) need
//               --filter FILE — every line a docID `d` or a half-open interval `lo:hi`, the filter their union
//               (doc_filter_file.hpp) — and each must be the only type of its run; a filtered type without --filter is a
//               usage error; also only with a wand file; the query lines, output and keys are ranked_or's;
//               ranked_or_faceted / ranked_and_faceted (dint_ranked_or_faceted_queries, dint_ranked_and_faceted_queries:
//               ranked_or / ranked_and with the matches counted per document group) need --facets FILE —
//               every line `d g` or `lo:hi g`, later lines win, a document no line names is in no group
//               (doc_facets_file.hpp) — take --filter FILE as an option, and each must be the only type of its run; a
//               faceted type without --facets is a usage error; also only with a wand file; the query lines, output and
//               keys are ranked_or's, and the JSON line carries besides "matches" (every match of the log),
//               "n_groups" and "facet_totals" (per group, the matches of the log's queries in it);
//               ranked_or_collapsed / ranked_and_collapsed (dint_ranked_or_collapsed_queries, dint_ranked_and_collapsed_queries:
//               of every document group a query matches only its best document is ranked) take
//               --facets FILE and --filter FILE as the faceted types do, and each must be the only type of its run; the
//               result counts are the hits (at most 10 groups a query), and the JSON line carries besides "matches" (every
//               match of the log), "collapsed" (the kept documents of the log's queries: groups with a match plus
//               ungrouped matches) and "n_groups";
//               ranked_or_paged / ranked_and_paged (dint_ranked_or_paged_queries, dint_ranked_and_paged_queries: search_after
//               paging) walk --pages N pages (default 2) of 10 hits per query, each page behind the last
//               hit of the one before; a query whose page comes back short is finished. --filter FILE is optional, and
//               --facets FILE selects the collapsed paged entries (pages of kept documents, one per group); each must be
//               the only type of its run; the result counts are the hits summed over the pages, and the JSON line carries
//               besides "pages", "hits" (the hits of the log's queries over their pages) and "matches" (every match of
//               the log; with --facets also "collapsed" and "n_groups"); --pages 1 answers what ranked_*_filtered answers;
//               ranked_or_group_limit / ranked_and_group_limit (dint_ranked_or_group_limit_queries,
//               dint_ranked_and_group_limit_queries: of every document group a query matches at most N documents are ranked,
//               DESIGN.md 4d-group-limit) need --facets FILE as the faceted types do and --per-group N (1 to 16), take
//               --filter FILE and --pages P (default 1: pages of 10 kept documents, each behind the last hit of the one
//               before), and each must be the only type of its run; the result counts are the hits summed over the pages,
//               and the JSON line carries besides "pages", "hits", "matches" (every match of the log), "kept" (the kept
//               documents of the log's queries), "per_group" and "n_groups"; --per-group 1 answers what ranked_*_paged
//               answers under the same --facets and --pages;
//               ranked_or_sorted / ranked_and_sorted (dint_ranked_or_sorted_queries, dint_ranked_and_sorted_queries: the matches
//               ordered by a per-document value) need --values FILE — every line `d v` or `lo:hi v`,
//               later lines win, a document no line names has value 0 (doc_values_file.hpp) — and take --order asc|desc
//               (default desc), --pages N (default 1: pages of 10 hits, each behind the last hit of the one before) and
//               either --filter FILE or --value-range lo:hi (the documents of the column whose value lies in the closed
//               interval, found on the device: dint_doc_filter_create_from_values), not both; each must be the only type
//               of its run; the result counts are the hits summed over the pages, and the JSON line carries besides
//               "pages", "hits", "matches" and "order";
//               ranked_or_value_stats / ranked_and_value_stats (dint_ranked_or_value_stats_queries,
//               dint_ranked_and_value_stats_queries: ranked_or / ranked_and with a column's values reduced over every match,
//               DESIGN.md 4d-stats) need --values FILE as the sorted types do and take --edges e1,e2,... — up to 1023 strictly
//               ascending decimal bucket boundaries (value_edges.hpp) — and either --filter FILE or --value-range lo:hi; each
//               must be the only type of its run; the query lines, output and keys are ranked_or's, and the JSON line carries
//               besides "matches", "value_n" and "value_sum" (totals over the log), "value_min" and "value_max" (over the
//               log; 4294967295 and 0 if no match has a value) and "buckets" (per bucket the log's total; [] without --edges);
//               ranked_or_group_stats / ranked_and_group_stats (dint_ranked_or_group_stats_queries,
//               dint_ranked_and_group_stats_queries: ranked_or / ranked_and with a column's values reduced over every match per
//               document group) need --facets FILE as the faceted types do and --values FILE as the
//               sorted types do, and take either --filter FILE or --value-range lo:hi; each must be the only type of its run;
//               the query lines, output and keys are ranked_or's, and the JSON line carries besides "matches", "n_groups" and
//               the per-group records merged over the log: "group_n", "group_sum", "group_min" and "group_max", arrays of
//               n_groups (4294967295 and 0 where no match of a group has a value);
//               ranked_or_percentiles / ranked_and_percentiles (dint_ranked_or_percentile_queries,
//               dint_ranked_and_percentile_queries: ranked_or / ranked_and with exact percentiles of a column's values over every
//               match) need --values FILE as the sorted types do and --percentiles p1,p2,... — 1 to 16
//               decimal percents between 0 and 100 with at most four fractional digits, in any order (percentile_list.hpp) — and
//               take either --filter FILE or --value-range lo:hi; each must be the only type of its run; the query lines, output
//               and keys are ranked_or's, and the JSON line carries besides "matches", "value_n" (the matches that have a
//               value, over the log), "per_million" (the ranks as parsed) and "percentile_sum" (per requested percentile the
//               sum of its values over the log's queries);
//               ranked_or_top_values / ranked_and_top_values (dint_ranked_or_top_values_queries,
//               dint_ranked_and_top_values_queries: ranked_or / ranked_and with the most frequent values of a column over every
//               match and the number of different ones) need --values FILE as the sorted types do and
//               --top-values N — 0 to 1024 values per query, 0: the counts only — and take either --filter FILE or
//               --value-range lo:hi; each must be the only type of its run; the query lines, output and keys are ranked_or's, and
//               the JSON line carries besides "matches", "value_n" (the matches that have a value), "distinct" (the different
//               values, query by query) and "top_count_sum" (the counts of the listed values), each summed over the log, and
//               "n_top";
//               wand and maxscore are out of scope and always print it
//   index_filename: what dint_create_freq_index wrote (dint/index_file.hpp)
//   wand_filename: what dint_create_wand_data wrote (include/dint_host.h), a positional argument as in src/queries.cpp:133-137
//   query_log on stdin: one query per line, term ids separated by blanks (include/ds2i/queries.hpp:15-27)
//
// Like op_perftest (src/queries.cpp:15-61): every query on its own, `runs` passes of which the first is not timed, the total
// of the result counts on stdout, then one stats line with the reference's keys — type, query, avg, q50, q90, q95 (µs). The
// device answers a BATCH per call much faster than a query per call: --batch times the whole log as one call
// and adds "batch_us_per_query" to the line.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <fstream>
#include <iostream>
#include <numeric>
#include <sstream>
#include <string>
#include <vector>

#include "dint/index_file.hpp"
#include "dint_hip.h"
#include "doc_facets_file.hpp"
#include "doc_filter_file.hpp"
#include "doc_values_file.hpp"
#include "tool_common.hpp"
#include "percentile_list.hpp"
#include "value_edges.hpp"

static void dint_ok(int st, const char* what) {
    if (st != DINT_OK) throw std::runtime_error(std::string(what) + ": " + dint_strerror(st) + " " + dint_last_hip_error());
}
static double now_us() {
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int main(int argc, char** argv) {
    if (argc < 4) {
        std::cerr << argv[0] << " <index_type> <query_type> <index_filename> [wand_filename] [--batch] [--runs R] [--filter FILE] [--facets FILE] [--pages N] [--per-group N] [--values FILE] [--order asc|desc] [--value-range lo:hi] [--edges e1,e2,...] [--percentiles p1,p2,...] [--top-values N] < query_log"
                  << std::endl;
        return 1;
    }
    try {
        std::string type = argv[1], query_type = argv[2];
        const char* index_filename = argv[3];
        const char* wand_filename = nullptr;
        const char* filter_filename = nullptr;
        const char* facets_filename = nullptr;
        const char* values_filename = nullptr;
        const char* value_range = nullptr;  // ranked_*_sorted: lo:hi, the run's filter from the column
        std::string order_name;             // ranked_*_sorted: asc | desc ("": not given)
        const char* edges_text = nullptr;   // ranked_*_value_stats: the bucket boundaries
        const char* percentiles_text = nullptr;  // ranked_*_percentiles: the ranks, in percent
        const char* top_values_text = nullptr;   // ranked_*_top_values: the values listed per query
        bool batch = false;
        size_t runs = 10 + 1;  // src/queries.cpp:13
        size_t pages = 0;      // ranked_*_paged: the pages walked per query (0: not given)
        long per_group = -1;   // ranked_*_group_limit: the hits a document group may show (-1: not given)
        for (int i = 4; i < argc; ++i) {
            std::string a = argv[i];
            if (a == "--batch") batch = true;
            else if (a == "--runs" && i + 1 < argc) runs = size_t(std::max(2, std::atoi(argv[++i])));
            else if (a == "--filter" && i + 1 < argc) filter_filename = argv[++i];
            else if (a == "--facets" && i + 1 < argc) facets_filename = argv[++i];
            else if (a == "--values" && i + 1 < argc) values_filename = argv[++i];
            else if (a == "--order" && i + 1 < argc) order_name = argv[++i];
            else if (a == "--value-range" && i + 1 < argc) value_range = argv[++i];
            else if (a == "--edges" && i + 1 < argc) edges_text = argv[++i];
            else if (a == "--percentiles" && i + 1 < argc) percentiles_text = argv[++i];
            else if (a == "--top-values" && i + 1 < argc) top_values_text = argv[++i];
            else if (a == "--pages" && i + 1 < argc) pages = size_t(std::max(1, std::atoi(argv[++i])));
            else if (a == "--per-group" && i + 1 < argc) per_group = std::max(0, std::atoi(argv[++i]));
            else if (!wand_filename && a.rfind("--", 0) != 0) wand_filename = argv[i];
            else throw std::runtime_error("unknown parameter");
        }
        const int kind = tool::kind_of_type(type);
        if (kind < 0) {
            std::cerr << "ERROR: Unknown type " << type << std::endl;  // src/queries.cpp:147-149
            return 0;
        }
        const bool is_bool = query_type == "ranked_bool";
        if (!is_bool && (":" + query_type + ":").find(":ranked_bool:") != std::string::npos)
            throw std::runtime_error("ranked_bool reads its query lines as +t / -t / t tokens: it must be the only query type of a run");
        const bool is_or_bool = query_type == "ranked_or_bool";
        if (!is_or_bool && (":" + query_type + ":").find(":ranked_or_bool:") != std::string::npos)
            throw std::runtime_error("ranked_or_bool reads its query lines as t / -t / ~m tokens: it must be the only query type of a run");
        const bool is_range = query_type == "ranked_or_range" || query_type == "ranked_and_range";
        for (const char* ranged : {"ranked_or_range", "ranked_and_range"})
            if (!is_range && (":" + query_type + ":").find(std::string(":") + ranged + ":") != std::string::npos)
                throw std::runtime_error(std::string(ranged) + " reads its query lines as term ids and one @lo:hi token: it must be the only query type of a run");
        const bool is_filtered = query_type == "ranked_or_filtered" || query_type == "ranked_and_filtered";
        for (const char* filtered : {"ranked_or_filtered", "ranked_and_filtered"})
            if (!is_filtered && (":" + query_type + ":").find(std::string(":") + filtered + ":") != std::string::npos)
                throw std::runtime_error(std::string(filtered) + " answers its whole log under --filter: it must be the only query type of a run");
        if (is_filtered && !filter_filename) {
            std::cerr << query_type << " needs --filter FILE (every line a docID d or an interval lo:hi)" << std::endl;
            return 1;
        }
        const bool is_collapsed = query_type == "ranked_or_collapsed" || query_type == "ranked_and_collapsed";
        const bool is_faceted = query_type == "ranked_or_faceted" || query_type == "ranked_and_faceted";
        const bool needs_facets = is_faceted || is_collapsed;  // the types that answer under the map of --facets
        for (const char* faceted : {"ranked_or_faceted", "ranked_and_faceted", "ranked_or_collapsed", "ranked_and_collapsed"})
            if (!needs_facets && (":" + query_type + ":").find(std::string(":") + faceted + ":") != std::string::npos)
                throw std::runtime_error(std::string(faceted) + " answers its whole log under --facets: it must be the only query type of a run");
        if (needs_facets && !facets_filename) {
            std::cerr << query_type << " needs --facets FILE (every line `d g` or `lo:hi g`: document d, or every document of [lo, hi), is in group g)"
                      << std::endl;
            return 1;
        }
        const bool is_paged = query_type == "ranked_or_paged" || query_type == "ranked_and_paged";
        for (const char* paged : {"ranked_or_paged", "ranked_and_paged"})
            if (!is_paged && (":" + query_type + ":").find(std::string(":") + paged + ":") != std::string::npos)
                throw std::runtime_error(std::string(paged) + " walks its whole log page by page: it must be the only query type of a run");
        const bool is_glimit = query_type == "ranked_or_group_limit" || query_type == "ranked_and_group_limit";
        for (const char* glimit : {"ranked_or_group_limit", "ranked_and_group_limit"})
            if (!is_glimit && (":" + query_type + ":").find(std::string(":") + glimit + ":") != std::string::npos)
                throw std::runtime_error(std::string(glimit) + " walks its whole log page by page under --facets: it must be the only query type of a run");
        if (is_glimit && !facets_filename) {
            std::cerr << query_type << " needs --facets FILE (every line `d g` or `lo:hi g`: document d, or every document of [lo, hi), is in group g)"
                      << std::endl;
            return 1;
        }
        if (is_glimit && per_group < 0) {
            std::cerr << query_type << " needs --per-group N (1 to " << DINT_GROUP_LIMIT_MAX << ": the hits a document group may show)" << std::endl;
            return 1;
        }
        if (!is_glimit && per_group >= 0) throw std::runtime_error("--per-group goes with ranked_or_group_limit and ranked_and_group_limit only");
        if (is_glimit && (per_group < 1 || per_group > DINT_GROUP_LIMIT_MAX))
            throw std::runtime_error("--per-group is 1 to " + std::to_string(DINT_GROUP_LIMIT_MAX));
        const bool is_sorted = query_type == "ranked_or_sorted" || query_type == "ranked_and_sorted";
        for (const char* sorted : {"ranked_or_sorted", "ranked_and_sorted"})
            if (!is_sorted && (":" + query_type + ":").find(std::string(":") + sorted + ":") != std::string::npos)
                throw std::runtime_error(std::string(sorted) + " walks its whole log page by page under --values: it must be the only query type of a run");
        const bool is_vstats = query_type == "ranked_or_value_stats" || query_type == "ranked_and_value_stats";
        for (const char* vstats : {"ranked_or_value_stats", "ranked_and_value_stats"})
            if (!is_vstats && (":" + query_type + ":").find(std::string(":") + vstats + ":") != std::string::npos)
                throw std::runtime_error(std::string(vstats) + " answers its whole log under --values: it must be the only query type of a run");
        const bool is_gstats = query_type == "ranked_or_group_stats" || query_type == "ranked_and_group_stats";
        for (const char* gstats : {"ranked_or_group_stats", "ranked_and_group_stats"})
            if (!is_gstats && (":" + query_type + ":").find(std::string(":") + gstats + ":") != std::string::npos)
                throw std::runtime_error(std::string(gstats) + " answers its whole log under --facets and --values: it must be the only query type of a run");
        const bool is_pct = query_type == "ranked_or_percentiles" || query_type == "ranked_and_percentiles";
        for (const char* pct : {"ranked_or_percentiles", "ranked_and_percentiles"})
            if (!is_pct && (":" + query_type + ":").find(std::string(":") + pct + ":") != std::string::npos)
                throw std::runtime_error(std::string(pct) + " answers its whole log under --values: it must be the only query type of a run");
        const bool is_topv = query_type == "ranked_or_top_values" || query_type == "ranked_and_top_values";
        for (const char* topv : {"ranked_or_top_values", "ranked_and_top_values"})
            if (!is_topv && (":" + query_type + ":").find(std::string(":") + topv + ":") != std::string::npos)
                throw std::runtime_error(std::string(topv) + " answers its whole log under --values: it must be the only query type of a run");
        if (is_gstats && !facets_filename) {
            std::cerr << query_type << " needs --facets FILE (every line `d g` or `lo:hi g`: document d, or every document of [lo, hi), is in group g)"
                      << std::endl;
            return 1;
        }
        if (!is_paged && !is_sorted && !is_glimit && pages) throw std::runtime_error("--pages goes with ranked_or_paged, ranked_and_paged, ranked_or_sorted and ranked_and_sorted only");
        if (is_paged && !pages) pages = 2;
        if ((is_sorted || is_glimit) && !pages) pages = 1;
        if (!is_sorted && !is_vstats && !is_gstats && !is_pct && !is_topv && (values_filename || value_range || !order_name.empty()))
            throw std::runtime_error("--values, --order and --value-range go with ranked_or_sorted and ranked_and_sorted only");
        if ((is_vstats || is_gstats || is_pct || is_topv) && !order_name.empty()) throw std::runtime_error("--order goes with ranked_or_sorted and ranked_and_sorted only");
        if (!is_vstats && edges_text) throw std::runtime_error("--edges goes with ranked_or_value_stats and ranked_and_value_stats only");
        if (!is_pct && percentiles_text) throw std::runtime_error("--percentiles goes with ranked_or_percentiles and ranked_and_percentiles only");
        if (!is_topv && top_values_text) throw std::runtime_error("--top-values goes with ranked_or_top_values and ranked_and_top_values only");
        if ((is_sorted || is_vstats || is_gstats || is_pct || is_topv) && !values_filename) {
            std::cerr << query_type << " needs --values FILE (every line `d v` or `lo:hi v`: document d, or every document of [lo, hi), has value v)"
                      << std::endl;
            return 1;
        }
        if (is_pct && !percentiles_text) {
            std::cerr << query_type << " needs --percentiles p1,p2,... (1 to 16 decimal percents between 0 and 100, at most four fractional digits)"
                      << std::endl;
            return 1;
        }
        uint32_t n_top = 0;
        if (is_topv) {
            const std::string digits = top_values_text ? top_values_text : "";
            if (digits.empty() || digits.size() > 4 || digits.find_first_not_of("0123456789") != std::string::npos ||
                std::stoul(digits) > DINT_TOP_VALUES_MAX) {
                std::cerr << query_type << " needs --top-values N (0 to " << DINT_TOP_VALUES_MAX << ": the values listed per query, 0: the counts only)"
                          << std::endl;
                return 1;
            }
            n_top = uint32_t(std::stoul(digits));
        }
        if (!order_name.empty() && order_name != "asc" && order_name != "desc") throw std::runtime_error("--order is asc or desc");
        const uint32_t sort_order = order_name == "asc" ? DINT_SORT_ASC : DINT_SORT_DESC;
        if (value_range && filter_filename) throw std::runtime_error("--value-range and --filter exclude each other: a run has one filter");
        if (is_sorted && facets_filename) throw std::runtime_error("--facets does not go with the ranked_*_sorted types");
        if (is_vstats && facets_filename) throw std::runtime_error("--facets does not go with the ranked_*_value_stats types");
        if (is_pct && facets_filename) throw std::runtime_error("--facets does not go with the ranked_*_percentiles types");
        if (is_topv && facets_filename) throw std::runtime_error("--facets does not go with the ranked_*_top_values types");
        std::vector<uint32_t> per_million;
        if (percentiles_text) per_million = tool::parse_percentiles(percentiles_text);
        std::vector<uint32_t> value_edges;
        if (edges_text) value_edges = tool::parse_value_edges(edges_text);
        uint32_t range_lo = 0, range_hi = 0;
        if (value_range) tool::parse_value_range(value_range, range_lo, range_hi);
        tool::doc_values_column values_column;
        if (is_sorted || is_vstats || is_gstats || is_pct || is_topv) {
            std::ifstream vf(values_filename);
            if (!vf) throw std::runtime_error(std::string("could not open the values file ") + values_filename);
            values_column = tool::parse_doc_values(vf);
        }
        if (!needs_facets && !is_paged && !is_gstats && !is_glimit && facets_filename)
            throw std::runtime_error("--facets goes with the ranked_*_faceted, ranked_*_collapsed and ranked_*_paged types only");
        if (!is_filtered && !needs_facets && !is_paged && !is_sorted && !is_vstats && !is_gstats && !is_pct && !is_topv && !is_glimit && filter_filename)
            throw std::runtime_error("--filter goes with the ranked_*_filtered, ranked_*_faceted, ranked_*_collapsed, ranked_*_paged and ranked_*_sorted types only");
        const bool uses_facets = needs_facets || is_gstats || is_glimit || (is_paged && facets_filename);  // (a paged type: the collapsed paged entry)
        tool::doc_facets_map facets_map;
        if (uses_facets) {
            std::ifstream ff(facets_filename);
            if (!ff) throw std::runtime_error(std::string("could not open the facets file ") + facets_filename);
            facets_map = tool::parse_doc_facets(ff);
        }
        tool::doc_filter_bits filter_bits;
        if (filter_filename) {
            std::ifstream ff(filter_filename);
            if (!ff) throw std::runtime_error(std::string("could not open the filter file ") + filter_filename);
            filter_bits = tool::parse_doc_filter(ff);
        }
        // read_query (queries.hpp:15-27)
        std::vector<std::vector<uint32_t>> queries;
        // ranked_bool: `queries` holds the required terms; the optional and excluded ones packed, offsets per query
        // ranked_or_bool: `queries` holds the optional terms; the excluded ones packed, and every line's minimum
        std::vector<uint32_t> should_terms, not_terms, mins;
        std::vector<uint64_t> should_offs(1, 0), not_offs(1, 0);
        std::vector<dint_doc_range> ranges;  // ranked_*_range: every line's range
        for (std::string line; std::getline(std::cin, line);) {
            std::istringstream iline(line);
            std::vector<uint32_t> q;
            if (is_bool) {
                for (std::string tok; iline >> tok;) {
                    const char sign = tok[0];
                    const std::string digits = sign == '+' || sign == '-' ? tok.substr(1) : tok;
                    if (digits.empty() || digits.find_first_not_of("0123456789") != std::string::npos || digits.size() > 10 ||
                        std::stoull(digits) > 0xFFFFFFFFull)
                        throw std::runtime_error("ranked_bool: not a term token: " + tok);
                    const uint32_t t = uint32_t(std::stoull(digits));
                    (sign == '+' ? q : sign == '-' ? not_terms : should_terms).push_back(t);
                }
                should_offs.push_back(should_terms.size());
                not_offs.push_back(not_terms.size());
            } else if (is_or_bool) {
                bool has_min = false;
                for (std::string tok; iline >> tok;) {
                    const char sign = tok[0];
                    if (sign == '+') throw std::runtime_error("ranked_or_bool: no required terms (+t): that query is ranked_bool's: " + tok);
                    const std::string digits = sign == '-' || sign == '~' ? tok.substr(1) : tok;
                    if (digits.empty() || digits.find_first_not_of("0123456789") != std::string::npos || digits.size() > 10 ||
                        std::stoull(digits) > 0xFFFFFFFFull || (sign == '~' && has_min))
                        throw std::runtime_error("ranked_or_bool: not a term token: " + tok);
                    const uint32_t t = uint32_t(std::stoull(digits));
                    if (sign == '~') has_min = true, mins.push_back(t);
                    else (sign == '-' ? not_terms : q).push_back(t);
                }
                if (!has_min) mins.push_back(1);
                not_offs.push_back(not_terms.size());
            } else if (is_range) {
                auto number = [&](const std::string& digits, const std::string& tok) {
                    if (digits.empty() || digits.find_first_not_of("0123456789") != std::string::npos || digits.size() > 10 ||
                        std::stoull(digits) > 0xFFFFFFFFull)
                        throw std::runtime_error(query_type + ": not a term id or an @lo:hi range: " + tok);
                    return uint32_t(std::stoull(digits));
                };
                bool has_range = false;
                dint_doc_range r{0u, 0xFFFFFFFFu};
                for (std::string tok; iline >> tok;) {
                    if (tok[0] != '@') {
                        q.push_back(number(tok, tok));
                        continue;
                    }
                    if (has_range) throw std::runtime_error(query_type + ": more than one @lo:hi range on a line: " + tok);
                    const size_t colon = tok.find(':');
                    if (colon == std::string::npos) throw std::runtime_error(query_type + ": not a term id or an @lo:hi range: " + tok);
                    r.lo = number(tok.substr(1, colon - 1), tok);
                    r.hi = number(tok.substr(colon + 1), tok);
                    has_range = true;
                }
                ranges.push_back(r);
            } else {
                for (uint32_t t; iline >> t;) q.push_back(t);
            }
            queries.push_back(q);
        }
        std::cerr << "Loading index from " << index_filename << std::endl;
        tool::mapped_file m(index_filename);
        const dint::index_file_view v = dint::view_index_file(m.data, m.bytes);
        if (int(v.header.kind) != kind) throw std::runtime_error("the index file holds another index type");
        const size_t n_lists = size_t(v.header.n_lists);
        for (auto const& q : queries)
            for (uint32_t t : q)
                if (t >= n_lists) throw std::runtime_error("query term " + std::to_string(t) + " is not a list of this index");
        for (auto const* clause : {&should_terms, &not_terms})
            for (uint32_t t : *clause)
                if (t >= n_lists) throw std::runtime_error("query term " + std::to_string(t) + " is not a list of this index");

        std::string device_name = "unknown";
        {
            hipDeviceProp_t prop;
            if (hipGetDeviceProperties(&prop, 0) == hipSuccess) device_name = prop.gcnArchName;  // e.g. gfx950:sramecc+:xnack-
        }
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
        dint_wand_data *wand = nullptr, *wand_blockmax = nullptr;  // (the second: with block maxima, for ranked_or_blockmax)
        if (wand_filename) {  // (the reference maps the wand data once, src/queries.cpp:84-89)
            tool::blob norm_lens, max_term_weight;
            tool::host_ok(dinth_read_wand_data(wand_filename, &norm_lens.h, &max_term_weight.h), "dinth_read_wand_data");
            dint_ok(dint_wand_data_create_with_max_weights(0, static_cast<const float*>(norm_lens.data()), norm_lens.size() / 4,
                                                           static_cast<const float*>(max_term_weight.data()), max_term_weight.size() / 4, &wand),
                    "dint_wand_data_create_with_max_weights");
            if ((":" + query_type + ":").find(":ranked_or_blockmax:") != std::string::npos) {
                dint_ok(dint_wand_data_create_with_max_weights(0, static_cast<const float*>(norm_lens.data()), norm_lens.size() / 4,
                                                               static_cast<const float*>(max_term_weight.data()), max_term_weight.size() / 4,
                                                               &wand_blockmax),
                        "dint_wand_data_create_with_max_weights");
                std::vector<float> term_max(n_lists), block_max(n_blocks);
                dint_ok(dint_index_max_weights(qi, freqs_dict, wand_blockmax, term_max.data(), block_max.data(), nullptr), "dint_index_max_weights");
                dint_ok(dint_wand_data_set_block_max_weights(wand_blockmax, block_max.data(), n_blocks), "dint_wand_data_set_block_max_weights");
            }
        }
        dint_doc_filter* doc_filter = nullptr;  // ranked_*_filtered: the run's filter
        if (filter_filename) dint_ok(dint_doc_filter_create(qi, filter_bits.words.data(), filter_bits.num_docs, &doc_filter), "dint_doc_filter_create");
        dint_doc_values* doc_values = nullptr;  // ranked_*_sorted, ranked_*_value_stats, ranked_*_group_stats: the run's column, and with --value-range the filter from it
        if (is_sorted || is_vstats || is_gstats || is_pct || is_topv) {
            dint_ok(dint_doc_values_create(0, values_column.values.data(), values_column.num_docs, &doc_values), "dint_doc_values_create");
            if (value_range) dint_ok(dint_doc_filter_create_from_values(qi, doc_values, range_lo, range_hi, &doc_filter), "dint_doc_filter_create_from_values");
        }
        dint_doc_facets* doc_facets = nullptr;  // ranked_*_faceted: the run's map, and a call's rows and matches
        if (uses_facets)
            dint_ok(dint_doc_facets_create(0, facets_map.group_of.data(), facets_map.num_docs, facets_map.n_groups, &doc_facets), "dint_doc_facets_create");
        const size_t n_groups = facets_map.n_groups;
        std::vector<uint32_t> facet_rows;
        std::vector<uint64_t> facet_matches;
        // ranked_*_collapsed: a call's kept documents; its hits' groups and group matches are outputs the ABI requires, and
        // the tool, which prints totals, does not read them
        std::vector<uint64_t> collapsed_counts;
        std::vector<uint32_t> hit_groups, hit_group_matches;
        // ranked_*_group_limit: its kept documents go where the collapsed types' do; the hits' places in their groups besides
        std::vector<uint32_t> hit_group_ranks;
        constexpr uint32_t kTopK = 10;  // ranked_and_query(wdata, 10), src/queries.cpp:106-108
        std::vector<float> top_scores;
        // ranked_*_paged: a page's docIDs and counts, and every query's cursor — the last hit of its page before
        std::vector<uint32_t> top_docids;
        std::vector<uint64_t> page_counts;
        std::vector<dint_rank_cursor> cursors;
        // ranked_*_sorted: a page's values beside them, and every query's cursor — (value, docid) of its last hit
        std::vector<uint32_t> top_values;
        std::vector<dint_value_cursor> value_cursors;
        // ranked_*_value_stats: a call's records and bucket rows
        std::vector<dint_value_stats> value_stats;
        std::vector<uint32_t> bucket_rows;
        const size_t n_buckets = value_edges.empty() ? 0 : value_edges.size() + 1;
        // ranked_*_group_stats: a call's records, n_groups per query
        std::vector<dint_value_stats> group_recs;
        // ranked_*_percentiles: a call's valued matches per query and its answers, n_pct per query
        std::vector<uint64_t> value_counts;
        std::vector<uint32_t> percentile_values;
        const size_t n_pct = per_million.size();
        // ranked_*_top_values: a call's distinct values and listed values per query (the valued matches go to value_counts), and
        // the lists themselves, n_top per query
        std::vector<uint64_t> distinct_counts;
        std::vector<uint32_t> top_ns, top_list_values, top_list_counts;

        std::vector<std::string> types;
        for (size_t a = 0; a <= query_type.size();) {
            size_t b = query_type.find(':', a);
            if (b == std::string::npos) b = query_type.size();
            types.push_back(query_type.substr(a, b - a));
            a = b + 1;
        }
        for (auto const& t : types) {
            const bool is_blockmax = t == "ranked_or_blockmax" && wand_blockmax;
            const bool is_maxscore = (t == "ranked_or_maxscore" && wand) || is_blockmax;
            const bool is_ranked_or = t == "ranked_or" && wand;
            const bool is_ranked_bool = t == "ranked_bool" && wand;
            const bool is_ranked_or_bool = t == "ranked_or_bool" && wand;
            const bool is_or_range = t == "ranked_or_range" && wand, is_and_range = t == "ranked_and_range" && wand;
            const bool is_or_filtered = t == "ranked_or_filtered" && wand, is_and_filtered = t == "ranked_and_filtered" && wand;
            const bool is_or_faceted = t == "ranked_or_faceted" && wand, is_and_faceted = t == "ranked_and_faceted" && wand;
            const bool is_or_collapsed = t == "ranked_or_collapsed" && wand, is_and_collapsed = t == "ranked_and_collapsed" && wand;
            const bool is_or_paged = t == "ranked_or_paged" && wand, is_and_paged = t == "ranked_and_paged" && wand;
            const bool is_or_glimit = t == "ranked_or_group_limit" && wand, is_and_glimit = t == "ranked_and_group_limit" && wand;
            const bool is_or_sorted = t == "ranked_or_sorted" && wand, is_and_sorted = t == "ranked_and_sorted" && wand;
            const bool is_or_vstats = t == "ranked_or_value_stats" && wand, is_and_vstats = t == "ranked_and_value_stats" && wand;
            const bool is_or_gstats = t == "ranked_or_group_stats" && wand, is_and_gstats = t == "ranked_and_group_stats" && wand;
            const bool is_or_pct = t == "ranked_or_percentiles" && wand, is_and_pct = t == "ranked_and_percentiles" && wand;
            const bool is_or_topv = t == "ranked_or_top_values" && wand, is_and_topv = t == "ranked_and_top_values" && wand;
            const bool is_ranked = (t == "ranked_and" && wand) || is_or_topv || is_and_topv || is_or_pct || is_and_pct || is_or_gstats || is_and_gstats || is_or_vstats || is_and_vstats || is_or_sorted || is_and_sorted || is_or_paged || is_and_paged || is_ranked_or || is_maxscore || is_ranked_bool || is_ranked_or_bool ||
                                   is_or_range || is_and_range || is_or_filtered || is_and_filtered || is_or_faceted || is_and_faceted ||
                                   is_or_collapsed || is_and_collapsed || is_or_glimit || is_and_glimit;
            if (t != "and" && t != "and_freq" && t != "or" && t != "or_freq" && !is_ranked) {
                std::cerr << "Unsupported query type: " << t << std::endl;  // src/queries.cpp:108-110
                continue;
            }
            const bool with_freqs = t == "and_freq" || t == "or_freq";
            const bool is_or = t == "or" || t == "or_freq";
            // one call of the query type's entry: n queries, packed (q0: the first of them in the log)
            auto run_queries = [&](const uint32_t* q_terms, const uint64_t* q_offs, size_t n, uint64_t* q_counts, uint64_t* q_fsums, size_t q0) {
                uint64_t fblocks = 0;
                if (is_ranked_bool) {
                    if (top_scores.size() < n * kTopK) top_scores.resize(n * kTopK);
                    dint_ok(dint_ranked_bool_queries(qi, freqs_dict, wand, kTopK, q_terms, q_offs, should_terms.data(), should_offs.data() + q0,
                                                     not_terms.data(), not_offs.data() + q0, n, q_counts, nullptr, top_scores.data(), nullptr,
                                                     nullptr, nullptr),
                            "dint_ranked_bool_queries");
                } else if (is_ranked_or_bool) {
                    if (top_scores.size() < n * kTopK) top_scores.resize(n * kTopK);
                    dint_ok(dint_ranked_or_bool_queries(qi, freqs_dict, wand, kTopK, q_terms, q_offs, not_terms.data(), not_offs.data() + q0,
                                                        mins.data() + q0, n, q_counts, nullptr, top_scores.data(), nullptr, nullptr, nullptr),
                            "dint_ranked_or_bool_queries");
                } else if (is_or_range || is_and_range) {
                    if (top_scores.size() < n * kTopK) top_scores.resize(n * kTopK);
                    if (is_or_range)
                        dint_ok(dint_ranked_or_range_queries(qi, freqs_dict, wand, kTopK, q_terms, q_offs, ranges.data() + q0, n, q_counts, nullptr,
                                                             top_scores.data(), nullptr, nullptr, nullptr),
                                "dint_ranked_or_range_queries");
                    else
                        dint_ok(dint_ranked_and_range_queries(qi, freqs_dict, wand, kTopK, q_terms, q_offs, ranges.data() + q0, n, q_counts, nullptr,
                                                              top_scores.data(), nullptr, nullptr, nullptr),
                                "dint_ranked_and_range_queries");
                } else if (is_or_filtered || is_and_filtered) {
                    if (top_scores.size() < n * kTopK) top_scores.resize(n * kTopK);
                    if (is_or_filtered)
                        dint_ok(dint_ranked_or_filtered_queries(qi, freqs_dict, wand, kTopK, q_terms, q_offs, doc_filter, n, q_counts, nullptr,
                                                                top_scores.data(), nullptr, nullptr, nullptr),
                                "dint_ranked_or_filtered_queries");
                    else
                        dint_ok(dint_ranked_and_filtered_queries(qi, freqs_dict, wand, kTopK, q_terms, q_offs, doc_filter, n, q_counts, nullptr,
                                                                 top_scores.data(), nullptr, nullptr, nullptr),
                                "dint_ranked_and_filtered_queries");
                } else if (is_or_faceted || is_and_faceted) {
                    if (top_scores.size() < n * kTopK) top_scores.resize(n * kTopK);
                    facet_rows.resize(n * n_groups);
                    facet_matches.resize(n);
                    if (is_or_faceted)
                        dint_ok(dint_ranked_or_faceted_queries(qi, freqs_dict, wand, kTopK, q_terms, q_offs, doc_filter, doc_facets, n, q_counts,
                                                               facet_matches.data(), top_scores.data(), nullptr, facet_rows.data(), nullptr, nullptr),
                                "dint_ranked_or_faceted_queries");
                    else
                        dint_ok(dint_ranked_and_faceted_queries(qi, freqs_dict, wand, kTopK, q_terms, q_offs, doc_filter, doc_facets, n, q_counts,
                                                                facet_matches.data(), top_scores.data(), nullptr, facet_rows.data(), nullptr, nullptr),
                                "dint_ranked_and_faceted_queries");
                } else if (is_or_collapsed || is_and_collapsed) {
                    if (top_scores.size() < n * kTopK) top_scores.resize(n * kTopK);
                    facet_matches.resize(n);
                    collapsed_counts.resize(n);
                    hit_groups.resize(n * kTopK);
                    hit_group_matches.resize(n * kTopK);
                    if (is_or_collapsed)
                        dint_ok(dint_ranked_or_collapsed_queries(qi, freqs_dict, wand, kTopK, q_terms, q_offs, doc_filter, doc_facets, n, q_counts,
                                                                 facet_matches.data(), collapsed_counts.data(), top_scores.data(), nullptr,
                                                                 hit_groups.data(), hit_group_matches.data(), nullptr, nullptr, nullptr),
                                "dint_ranked_or_collapsed_queries");
                    else
                        dint_ok(dint_ranked_and_collapsed_queries(qi, freqs_dict, wand, kTopK, q_terms, q_offs, doc_filter, doc_facets, n, q_counts,
                                                                  facet_matches.data(), collapsed_counts.data(), top_scores.data(), nullptr,
                                                                  hit_groups.data(), hit_group_matches.data(), nullptr, nullptr, nullptr),
                                "dint_ranked_and_collapsed_queries");
                } else if (is_or_paged || is_and_paged || is_or_glimit || is_and_glimit) {
                    if (top_scores.size() < n * kTopK) top_scores.resize(n * kTopK);
                    top_docids.resize(n * kTopK);
                    page_counts.resize(n);
                    facet_matches.resize(n);
                    cursors.assign(n, dint_rank_cursor{INFINITY, 0u});  // (from the start)
                    std::fill(q_counts, q_counts + n, uint64_t(0));
                    if (doc_facets) {
                        collapsed_counts.resize(n);
                        hit_groups.resize(n * kTopK);
                        hit_group_matches.resize(n * kTopK);
                        hit_group_ranks.resize(n * kTopK);
                    }
                    for (size_t page = 0; page != pages; ++page) {
                        if (is_or_glimit || is_and_glimit)
                            dint_ok((is_or_glimit ? dint_ranked_or_group_limit_queries : dint_ranked_and_group_limit_queries)(
                                        qi, freqs_dict, wand, kTopK, q_terms, q_offs, doc_filter, doc_facets, uint32_t(per_group), cursors.data(), n,
                                        page_counts.data(), facet_matches.data(), collapsed_counts.data(), nullptr, top_scores.data(),
                                        top_docids.data(), hit_groups.data(), hit_group_matches.data(), hit_group_ranks.data(), nullptr, nullptr,
                                        nullptr),
                                    "dint_ranked_*_group_limit_queries");
                        else if (doc_facets)
                            dint_ok((is_or_paged ? dint_ranked_or_collapsed_paged_queries : dint_ranked_and_collapsed_paged_queries)(
                                        qi, freqs_dict, wand, kTopK, q_terms, q_offs, doc_filter, doc_facets, cursors.data(), n, page_counts.data(),
                                        facet_matches.data(), collapsed_counts.data(), nullptr, top_scores.data(), top_docids.data(),
                                        hit_groups.data(), hit_group_matches.data(), nullptr, nullptr, nullptr),
                                    "dint_ranked_*_collapsed_paged_queries");
                        else
                            dint_ok((is_or_paged ? dint_ranked_or_paged_queries : dint_ranked_and_paged_queries)(
                                        qi, freqs_dict, wand, kTopK, q_terms, q_offs, doc_filter, cursors.data(), n, page_counts.data(),
                                        facet_matches.data(), nullptr, top_scores.data(), top_docids.data(), nullptr, nullptr),
                                    "dint_ranked_*_paged_queries");
                        bool more = false;
                        for (size_t q = 0; q != n; ++q) {
                            q_counts[q] += page_counts[q];
                            // a full page: the next one begins behind its last hit; a short one: the query is finished, and a
                            // cursor of score 0 leaves nothing after it
                            if (page_counts[q] == kTopK) {
                                cursors[q] = dint_rank_cursor{top_scores[q * kTopK + kTopK - 1], top_docids[q * kTopK + kTopK - 1]};
                                more = true;
                            } else {
                                cursors[q] = dint_rank_cursor{0.0f, 0u};
                            }
                        }
                        if (!more) break;
                    }
                } else if (is_or_sorted || is_and_sorted) {
                    top_values.resize(n * kTopK);
                    top_docids.resize(n * kTopK);
                    page_counts.resize(n);
                    facet_matches.resize(n);
                    value_cursors.assign(n, dint_value_cursor{0u, 0u, 0u});  // (from the start)
                    std::fill(q_counts, q_counts + n, uint64_t(0));
                    std::vector<char> finished(n, 0);
                    for (size_t page = 0; page != pages; ++page) {
                        dint_ok((is_or_sorted ? dint_ranked_or_sorted_queries : dint_ranked_and_sorted_queries)(
                                    qi, freqs_dict, wand, kTopK, q_terms, q_offs, doc_filter, doc_values, sort_order, value_cursors.data(), n,
                                    page_counts.data(), facet_matches.data(), nullptr, top_values.data(), top_docids.data(), nullptr, nullptr,
                                    nullptr),
                                "dint_ranked_*_sorted_queries");
                        bool more = false;
                        for (size_t q = 0; q != n; ++q) {
                            if (finished[q]) continue;  // (a short page ended the query: what later calls return for it is not counted)
                            q_counts[q] += page_counts[q];
                            if (page_counts[q] == kTopK) {
                                value_cursors[q] = dint_value_cursor{top_values[q * kTopK + kTopK - 1], top_docids[q * kTopK + kTopK - 1], 1u};
                                more = true;
                            } else {
                                finished[q] = 1;
                            }
                        }
                        if (!more) break;
                    }
                } else if (is_or_vstats || is_and_vstats) {
                    if (top_scores.size() < n * kTopK) top_scores.resize(n * kTopK);
                    facet_matches.resize(n);
                    value_stats.resize(n);
                    bucket_rows.resize(n * n_buckets);
                    dint_ok((is_or_vstats ? dint_ranked_or_value_stats_queries : dint_ranked_and_value_stats_queries)(
                                qi, freqs_dict, wand, kTopK, q_terms, q_offs, doc_filter, doc_values, value_edges.data(), uint32_t(value_edges.size()),
                                n, q_counts, facet_matches.data(), top_scores.data(), nullptr, value_stats.data(), bucket_rows.data(), nullptr,
                                nullptr, nullptr),
                            "dint_ranked_*_value_stats_queries");
                } else if (is_or_gstats || is_and_gstats) {
                    if (top_scores.size() < n * kTopK) top_scores.resize(n * kTopK);
                    facet_matches.resize(n);
                    group_recs.resize(n * n_groups);
                    dint_ok((is_or_gstats ? dint_ranked_or_group_stats_queries : dint_ranked_and_group_stats_queries)(
                                qi, freqs_dict, wand, kTopK, q_terms, q_offs, doc_filter, doc_facets, doc_values, n, q_counts, facet_matches.data(),
                                top_scores.data(), nullptr, group_recs.data(), nullptr, nullptr, nullptr),
                            "dint_ranked_*_group_stats_queries");
                } else if (is_or_pct || is_and_pct) {
                    if (top_scores.size() < n * kTopK) top_scores.resize(n * kTopK);
                    facet_matches.resize(n);
                    value_counts.resize(n);
                    percentile_values.resize(n * n_pct);
                    // (a call takes at most DINT_PERCENTILES_MAX_RECORDS (query, percentile) pairs: a longer log goes in parts)
                    const size_t most = size_t(DINT_PERCENTILES_MAX_RECORDS / n_pct);
                    for (size_t at = 0; at < n; at += most) {
                        const size_t part = std::min(most, n - at);
                        dint_ok((is_or_pct ? dint_ranked_or_percentile_queries : dint_ranked_and_percentile_queries)(
                                    qi, freqs_dict, wand, kTopK, q_terms, q_offs + at, doc_filter, doc_values, per_million.data(), uint32_t(n_pct), part,
                                    q_counts + at, facet_matches.data() + at, top_scores.data() + at * kTopK, nullptr, value_counts.data() + at,
                                    percentile_values.data() + at * n_pct, nullptr, nullptr, nullptr),
                                "dint_ranked_*_percentile_queries");
                    }
                } else if (is_or_topv || is_and_topv) {
                    if (top_scores.size() < n * kTopK) top_scores.resize(n * kTopK);
                    facet_matches.resize(n);
                    value_counts.resize(n);
                    distinct_counts.resize(n);
                    top_ns.resize(n);
                    top_list_values.resize(n * n_top);
                    top_list_counts.resize(n * n_top);
                    dint_ok((is_or_topv ? dint_ranked_or_top_values_queries : dint_ranked_and_top_values_queries)(
                                qi, freqs_dict, wand, kTopK, q_terms, q_offs, doc_filter, doc_values, n_top, n, q_counts, facet_matches.data(),
                                top_scores.data(), nullptr, value_counts.data(), distinct_counts.data(), top_ns.data(),
                                n_top ? top_list_values.data() : nullptr, n_top ? top_list_counts.data() : nullptr, nullptr, nullptr),
                            "dint_ranked_*_top_values_queries");
                } else if (is_maxscore) {
                    if (top_scores.size() < n * kTopK) top_scores.resize(n * kTopK);
                    dint_ok(dint_ranked_or_maxscore_queries(qi, freqs_dict, is_blockmax ? wand_blockmax : wand, kTopK, q_terms, q_offs, n, q_counts, top_scores.data(), nullptr,
                                                            nullptr, nullptr),
                            "dint_ranked_or_maxscore_queries");
                } else if (is_ranked_or) {
                    if (top_scores.size() < n * kTopK) top_scores.resize(n * kTopK);
                    dint_ok(dint_ranked_or_queries(qi, freqs_dict, wand, kTopK, q_terms, q_offs, n, q_counts, top_scores.data(), nullptr, nullptr),
                            "dint_ranked_or_queries");
                } else if (is_ranked) {
                    if (top_scores.size() < n * kTopK) top_scores.resize(n * kTopK);
                    dint_ok(dint_ranked_and_queries(qi, freqs_dict, wand, kTopK, q_terms, q_offs, n, q_counts, top_scores.data(), nullptr, nullptr),
                            "dint_ranked_and_queries");
                } else if (is_or && with_freqs)
                    dint_ok(dint_or_queries_freqs(qi, freqs_dict, q_terms, q_offs, n, q_counts, q_fsums, &fblocks, nullptr), "dint_or_queries_freqs");
                else if (is_or)
                    dint_ok(dint_or_queries(qi, q_terms, q_offs, n, q_counts, nullptr), "dint_or_queries");
                else if (with_freqs)
                    dint_ok(dint_and_queries_freqs(qi, freqs_dict, q_terms, q_offs, n, q_counts, q_fsums, &fblocks, nullptr), "dint_and_queries_freqs");
                else
                    dint_ok(dint_and_queries(qi, q_terms, q_offs, n, q_counts, nullptr), "dint_and_queries");
            };
            std::vector<double> query_times;
            uint64_t total = 0, total_one_run = 0;
            // a faceted type: per group the matches of the log's queries in it, and every match of the log (the first run's)
            std::vector<uint64_t> facet_totals(is_faceted ? n_groups : 0, 0);
            uint64_t all_matches = 0, all_collapsed = 0;  // (a collapsed type: every kept document of the log besides)
            // a value-stats type: the log's records merged and per bucket the log's total (the first run's)
            dint_value_stats log_stats{0, 0, 0xFFFFFFFFu, 0};
            std::vector<uint64_t> bucket_totals(is_vstats ? n_buckets : 0, 0);
            auto merge_stats = [&](dint_value_stats& into, std::vector<uint64_t>& buckets, size_t n) {
                for (size_t q = 0; q != n; ++q) {
                    into.n += value_stats[q].n;
                    into.sum += value_stats[q].sum;
                    into.min = std::min(into.min, value_stats[q].min);
                    into.max = std::max(into.max, value_stats[q].max);
                    for (size_t b = 0; b != n_buckets; ++b) buckets[b] += bucket_rows[q * n_buckets + b];
                }
            };
            // a group-stats type: per group the log's records merged (the first run's)
            std::vector<dint_value_stats> group_totals(is_gstats ? n_groups : 0, dint_value_stats{0, 0, 0xFFFFFFFFu, 0});
            auto merge_groups = [&](std::vector<dint_value_stats>& into, size_t n) {
                for (size_t q = 0; q != n; ++q)
                    for (size_t g = 0; g != n_groups; ++g) {
                        const dint_value_stats& r = group_recs[q * n_groups + g];
                        into[g].n += r.n;
                        into[g].sum += r.sum;
                        into[g].min = std::min(into[g].min, r.min);
                        into[g].max = std::max(into[g].max, r.max);
                    }
            };
            // a percentile type: the log's valued matches and per requested percentile the sum of its values (the first run's)
            uint64_t log_value_n = 0;
            std::vector<uint64_t> percentile_sums(is_pct ? n_pct : 0, 0);
            auto merge_percentiles = [&](uint64_t& into_n, std::vector<uint64_t>& sums, size_t n) {
                for (size_t q = 0; q != n; ++q) {
                    into_n += value_counts[q];
                    for (size_t j = 0; j != n_pct; ++j) sums[j] += percentile_values[q * n_pct + j];
                }
            };
            // a top-values type: the log's valued matches, distinct values (query by query) and listed counts (the first run's)
            uint64_t log_distinct = 0, log_top_counts = 0;
            auto merge_top_values = [&](uint64_t& into_n, uint64_t& into_distinct, uint64_t& into_counts, size_t n) {
                for (size_t q = 0; q != n; ++q) {
                    into_n += value_counts[q];
                    into_distinct += distinct_counts[q];
                    for (size_t i = 0; i != top_ns[q]; ++i) into_counts += top_list_counts[q * n_top + i];
                }
            };
            for (size_t run = 0; run != runs; ++run) {  // op_perftest
                for (size_t i = 0; i != queries.size(); ++i) {
                    auto const& q = queries[i];
                    const uint64_t offs[2] = {0, q.size()};
                    uint64_t results = 0, fsum = 0;
                    const double tick = now_us();
                    run_queries(q.data(), offs, 1, &results, &fsum, i);
                    total += results;
                    if (run == 0) total_one_run += results;
                    if (run == 0 && is_vstats && is_ranked) merge_stats(log_stats, bucket_totals, 1);
                    if (run == 0 && is_gstats && is_ranked) merge_groups(group_totals, 1);
                    if (run == 0 && is_pct && is_ranked) merge_percentiles(log_value_n, percentile_sums, 1);
                    if (run == 0 && is_topv && is_ranked) merge_top_values(log_value_n, log_distinct, log_top_counts, 1);
                    if (run == 0 && (needs_facets || is_paged || is_glimit || is_sorted || is_vstats || is_gstats || is_pct || is_topv)) {
                        all_matches += facet_matches[0];
                        if (is_collapsed || is_glimit || (is_paged && doc_facets)) all_collapsed += collapsed_counts[0];
                        for (size_t g = 0; g != facet_totals.size(); ++g) facet_totals[g] += facet_rows[g];
                    }
                    if (run != 0) query_times.push_back(now_us() - tick);  // first run is not timed
                }
            }
            std::cout << total << std::endl;
            double batch_us = -1;
            if (batch && !queries.empty()) {
                std::vector<uint32_t> terms;
                std::vector<uint64_t> offs(1, 0), counts(queries.size(), 0), fsums(queries.size(), 0);
                for (auto const& q : queries) {
                    terms.insert(terms.end(), q.begin(), q.end());
                    offs.push_back(terms.size());
                }
                double best = 1e300;
                for (size_t run = 0; run != std::min<size_t>(runs, 4); ++run) {
                    const double tick = now_us();
                    run_queries(terms.data(), offs.data(), queries.size(), counts.data(), fsums.data(), 0);
                    if (run != 0) best = std::min(best, now_us() - tick);
                }
                batch_us = best / double(queries.size());
                // the batch call and the one-query calls answer the same log
                uint64_t batch_total = 0;
                for (uint64_t c : counts) batch_total += c;
                if (batch_total != total_one_run)
                    throw std::runtime_error("the batch call counted " + std::to_string(batch_total) + " results, the one-query calls " +
                                             std::to_string(total_one_run));
                if (is_collapsed || is_paged || is_glimit || is_sorted) {  // ... and keep the same documents
                    uint64_t batch_matches = 0, batch_collapsed = 0;
                    for (size_t q = 0; q != queries.size(); ++q)
                        batch_matches += facet_matches[q], batch_collapsed += is_collapsed || doc_facets ? collapsed_counts[q] : 0;
                    if (batch_matches != all_matches || batch_collapsed != all_collapsed)
                        throw std::runtime_error("the batch call and the one-query calls counted other matches or kept other documents");
                } else if (is_vstats) {  // ... and reduce the same values
                    dint_value_stats batch_stats{0, 0, 0xFFFFFFFFu, 0};
                    std::vector<uint64_t> batch_buckets(n_buckets, 0);
                    merge_stats(batch_stats, batch_buckets, queries.size());
                    uint64_t batch_matches = 0;
                    for (size_t q = 0; q != queries.size(); ++q) batch_matches += facet_matches[q];
                    if (batch_matches != all_matches || batch_stats.n != log_stats.n || batch_stats.sum != log_stats.sum ||
                        batch_stats.min != log_stats.min || batch_stats.max != log_stats.max || batch_buckets != bucket_totals)
                        throw std::runtime_error("the batch call and the one-query calls reduced other values");
                } else if (is_pct) {  // ... and select the same values
                    uint64_t batch_value_n = 0, batch_matches = 0;
                    std::vector<uint64_t> batch_sums(n_pct, 0);
                    merge_percentiles(batch_value_n, batch_sums, queries.size());
                    for (size_t q = 0; q != queries.size(); ++q) batch_matches += facet_matches[q];
                    if (batch_matches != all_matches || batch_value_n != log_value_n || batch_sums != percentile_sums)
                        throw std::runtime_error("the batch call and the one-query calls selected other percentiles");
                } else if (is_topv) {  // ... and count the same values
                    uint64_t batch_value_n = 0, batch_distinct = 0, batch_top_counts = 0, batch_matches = 0;
                    merge_top_values(batch_value_n, batch_distinct, batch_top_counts, queries.size());
                    for (size_t q = 0; q != queries.size(); ++q) batch_matches += facet_matches[q];
                    if (batch_matches != all_matches || batch_value_n != log_value_n || batch_distinct != log_distinct ||
                        batch_top_counts != log_top_counts)
                        throw std::runtime_error("the batch call and the one-query calls counted other values");
                } else if (is_gstats) {  // ... and reduce the same values per group
                    std::vector<dint_value_stats> batch_groups(n_groups, dint_value_stats{0, 0, 0xFFFFFFFFu, 0});
                    merge_groups(batch_groups, queries.size());
                    uint64_t batch_matches = 0;
                    for (size_t q = 0; q != queries.size(); ++q) batch_matches += facet_matches[q];
                    bool same = batch_matches == all_matches;
                    for (size_t g = 0; g != n_groups; ++g)
                        same = same && batch_groups[g].n == group_totals[g].n && batch_groups[g].sum == group_totals[g].sum &&
                               batch_groups[g].min == group_totals[g].min && batch_groups[g].max == group_totals[g].max;
                    if (!same) throw std::runtime_error("the batch call and the one-query calls reduced other values per group");
                } else if (is_faceted) {  // ... and count the same matches per group
                    std::vector<uint64_t> batch_totals(n_groups, 0);
                    for (size_t q = 0; q != queries.size(); ++q)
                        for (size_t g = 0; g != n_groups; ++g) batch_totals[g] += facet_rows[q * n_groups + g];
                    if (batch_totals != facet_totals) throw std::runtime_error("the batch call and the one-query calls counted other facet totals");
                }
            }
            if (query_times.empty()) continue;
            std::sort(query_times.begin(), query_times.end());
            const double avg = std::accumulate(query_times.begin(), query_times.end(), double()) / double(query_times.size());
            const double q50 = query_times[query_times.size() / 2], q90 = query_times[90 * query_times.size() / 100],
                         q95 = query_times[95 * query_times.size() / 100];
            std::cout << "{\"type\": \"" << type << "\", \"query\": \"" << t << "\", \"avg\": " << avg << ", \"q50\": " << q50
                      << ", \"q90\": " << q90 << ", \"q95\": " << q95;
            if (batch_us >= 0) std::cout << ", \"batch_us_per_query\": " << batch_us;
            if (is_gstats) {
                std::cout << ", \"matches\": " << all_matches << ", \"n_groups\": " << n_groups;
                auto column = [&](const char* key, auto field) {
                    std::cout << ", \"" << key << "\": [";
                    for (size_t g = 0; g != n_groups; ++g) std::cout << (g ? ", " : "") << field(group_totals[g]);
                    std::cout << "]";
                };
                column("group_n", [](const dint_value_stats& r) { return r.n; });
                column("group_sum", [](const dint_value_stats& r) { return r.sum; });
                column("group_min", [](const dint_value_stats& r) { return uint64_t(r.min); });
                column("group_max", [](const dint_value_stats& r) { return uint64_t(r.max); });
            } else if (is_pct) {
                std::cout << ", \"matches\": " << all_matches << ", \"value_n\": " << log_value_n << ", \"per_million\": [";
                for (size_t j = 0; j != n_pct; ++j) std::cout << (j ? ", " : "") << per_million[j];
                std::cout << "], \"percentile_sum\": [";
                for (size_t j = 0; j != n_pct; ++j) std::cout << (j ? ", " : "") << percentile_sums[j];
                std::cout << "]";
            } else if (is_topv) {
                std::cout << ", \"matches\": " << all_matches << ", \"value_n\": " << log_value_n << ", \"distinct\": " << log_distinct
                          << ", \"top_count_sum\": " << log_top_counts << ", \"n_top\": " << n_top;
            } else if (is_vstats) {
                std::cout << ", \"matches\": " << all_matches << ", \"value_n\": " << log_stats.n << ", \"value_sum\": " << log_stats.sum
                          << ", \"value_min\": " << log_stats.min << ", \"value_max\": " << log_stats.max << ", \"buckets\": [";
                for (size_t b = 0; b != n_buckets; ++b) std::cout << (b ? ", " : "") << bucket_totals[b];
                std::cout << "]";
            } else if (is_sorted) {
                std::cout << ", \"pages\": " << pages << ", \"hits\": " << total_one_run << ", \"matches\": " << all_matches << ", \"order\": \""
                          << (sort_order == DINT_SORT_ASC ? "asc" : "desc") << "\"";
            } else if (is_glimit) {
                std::cout << ", \"pages\": " << pages << ", \"hits\": " << total_one_run << ", \"matches\": " << all_matches << ", \"kept\": "
                          << all_collapsed << ", \"per_group\": " << per_group << ", \"n_groups\": " << n_groups;
            } else if (is_paged) {
                std::cout << ", \"pages\": " << pages << ", \"hits\": " << total_one_run << ", \"matches\": " << all_matches;
                if (doc_facets) std::cout << ", \"collapsed\": " << all_collapsed << ", \"n_groups\": " << n_groups;
            } else if (is_collapsed) {
                std::cout << ", \"matches\": " << all_matches << ", \"collapsed\": " << all_collapsed << ", \"n_groups\": " << n_groups;
            } else if (is_faceted) {
                std::cout << ", \"matches\": " << all_matches << ", \"n_groups\": " << n_groups << ", \"facet_totals\": [";
                for (size_t g = 0; g != n_groups; ++g) std::cout << (g ? ", " : "") << facet_totals[g];
                std::cout << "]";
            }
            std::cout << ", \"device\": \"" << device_name << "\"}" << std::endl;
        }
        dint_doc_facets_destroy(doc_facets);
        dint_doc_filter_destroy(doc_filter);
        dint_doc_values_destroy(doc_values);
        dint_wand_data_destroy(wand);
        dint_wand_data_destroy(wand_blockmax);
        dint_query_index_destroy(qi);
        dint_free(blocks);
        (void)hipFree(d_index);
        dint_dict_destroy(docs_dict);
        dint_dict_destroy(freqs_dict);
    } catch (std::exception const& e) {
        std::cerr << "ERROR: " << e.what() << std::endl;
        return 1;
    }
    return 0;
}
