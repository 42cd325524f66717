// C ABI of the device decode path (include/dint_hip.h): dictionary staging, the host indexing pre-pass, and the kernel
// launches. ONE translation unit (the kernels are templates in headers; the handles are shared): its parts live under
// host/ by subsystem and are included here in order — common helpers, handles and the query calls' staged layouts first,
// then the extern "C" block (opened in host/hip_api_common.inc, closed at the end of this file): dictionary, vroom
// decode, in-index decode, the query index and its page decodes, query planning, AND, OR, ranked AND, ranked OR and
// pruned ranked OR queries, docID-range, document-filter, faceted, collapsed, paged, group-limited, sorted, value-stats, group-stats, percentile and top-values ranked queries, scores of given documents, maxima from the index, the index checked against its collection,
// statistics, host-pointer calls, list cache.
#include "dint_hip.h"

#include <hip/hip_runtime.h>

#include <cstring>  // (before rocPRIM: one of its headers calls the host memset without including it)
#include <rocprim/device/device_merge_sort.hpp>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <mutex>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "dint_kernels.hpp"
#include "dint_query_kernels.hpp"
#include "dint_or_query_kernels.hpp"
#include "dint_ranked_query_kernels.hpp"
#include "dint_ranked_bool_kernels.hpp"
#include "dint_ranked_or_query_kernels.hpp"
#include "dint_ranked_or_bool_kernels.hpp"
#include "dint_ranked_or_maxscore_kernels.hpp"
#include "dint_ranked_range_kernels.hpp"
#include "dint_doc_filter_kernels.hpp"
#include "dint_facet_kernels.hpp"
#include "dint_collapse_kernels.hpp"
#include "dint_paging_kernels.hpp"
#include "dint_group_limit_kernels.hpp"
#include "dint_doc_values_kernels.hpp"
#include "dint_value_stats_kernels.hpp"
#include "dint_group_stats_kernels.hpp"
#include "dint_percentile_kernels.hpp"
#include "dint_top_values_kernels.hpp"
#include "dint_score_documents_kernels.hpp"
#include "dint_wand_kernels.hpp"
#include "dint_check_kernels.hpp"
#include "dint_stats_kernels.hpp"

#include "host/hip_common.inc"
#include "host/hip_handles.inc"
#include "host/hip_dictionary.inc"
#include "host/hip_stage_layout.inc"
#include "host/hip_query_handle.inc"
#include "host/hip_api_common.inc"
#include "host/hip_api_dictionary.inc"
#include "host/hip_api_vroom.inc"
#include "host/hip_api_index.inc"
#include "host/hip_api_query.inc"
#include "host/hip_api_query_plan.inc"
#include "host/hip_api_query_and.inc"
#include "host/hip_api_or_query.inc"
#include "host/hip_api_ranked_query.inc"
#include "host/hip_api_ranked_bool.inc"
#include "host/hip_api_ranked_or_query.inc"
#include "host/hip_api_ranked_or_bool.inc"
#include "host/hip_api_ranked_or_maxscore.inc"
#include "host/hip_api_ranked_range.inc"
#include "host/hip_api_doc_filter.inc"
#include "host/hip_api_facets.inc"
#include "host/hip_api_collapse.inc"
#include "host/hip_api_paging.inc"
#include "host/hip_api_group_limit.inc"
#include "host/hip_api_doc_values.inc"
#include "host/hip_api_value_stats.inc"
#include "host/hip_api_group_stats.inc"
#include "host/hip_api_percentiles.inc"
#include "host/hip_api_top_values.inc"
#include "host/hip_api_score_documents.inc"
#include "host/hip_api_wand.inc"
#include "host/hip_api_check.inc"
#include "host/hip_api_stats.inc"
#include "host/hip_api_host_calls.inc"
#include "host/hip_api_list_cache.inc"

int dint_debug_alloc_count(uint64_t* count) {
    if (!count) return DINT_ERR_ARG;
    *count = g_alloc_count.load();
    return DINT_OK;
}

#ifdef DINT_PROFILE
}  // extern "C"
#include "dint_profile_host.inc"
extern "C" {
#endif

// Test hook (not part of the decode ABI): inclusive wave prefix sum of 64 host words.
int dint_debug_wave_scan(const uint32_t* in64, uint32_t* out64) {
    if (!in64 || !out64) return DINT_ERR_ARG;
    uint32_t *d_in = nullptr, *d_out = nullptr;
    HIP_TRY(counted_malloc(&d_in, 256));
    HIP_TRY(counted_malloc(&d_out, 256));
    HIP_TRY(hipMemcpy(d_in, in64, 256, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(debug_wave_scan_kernel, dim3(1), dim3(64), 0, nullptr, d_in, d_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out64, d_out, 256, hipMemcpyDeviceToHost));
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    return DINT_OK;
}

}  // extern "C"

