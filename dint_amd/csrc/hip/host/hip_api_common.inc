// Part of dint_hip.hip (one translation unit; included from there, in order): extern "C": options, ABI version, status text, device count.
// ---- options (dint_set_option): process-wide switches for tests and measurements, read by the entry points with one
// relaxed atomic load — no environment variable is looked at anywhere in this library -----------------------------------
namespace {
struct option_def {
    const char* key;
    long long def;
};
// (the switches 0 .. DINT_OPT_COUNT_ - 1, then the workspace bounds, numbered apart in the header: option_slot)
constexpr int kOptionSlots = DINT_OPT_COUNT_ + 1;
constexpr option_def kOptionDefs[kOptionSlots] = {
    {"bundles", 1},                 // DINT_OPT_BUNDLES
    {"index_concurrent", 1},        // DINT_OPT_INDEX_CONCURRENT
    {"query_lean_pages", -1},       // DINT_OPT_QUERY_LEAN_PAGES (-1: every page decode takes the one-launch form)
    {"query_tail_pages", 4},        // DINT_OPT_QUERY_TAIL_PAGES
    {"query_fused_pages", 2},       // DINT_OPT_QUERY_FUSED_PAGES
    {"index_inline_tails", 1},      // DINT_OPT_INDEX_INLINE_TAILS
    {"chunk_split", -1},            // DINT_OPT_CHUNK_SPLIT
    {"index_pair", 1},              // DINT_OPT_INDEX_PAIR
    {"query_fused_copy", 1},        // DINT_OPT_QUERY_FUSED_COPY
    {"query_batch_fused", 1},       // DINT_OPT_QUERY_BATCH_FUSED
    {"split_units", 1},             // DINT_OPT_SPLIT_UNITS
    {"refine_units", 1},            // DINT_OPT_REFINE_UNITS
    {"query_or_pass_pages", 1 << 20},  // DINT_OPT_QUERY_OR_PASS_PAGES (1 GiB of docIDs a pass)
};
std::atomic<long long> g_options[kOptionSlots] = {{1}, {1}, {-1}, {4}, {2}, {1}, {-1}, {1}, {1}, {1}, {1}, {1}, {1 << 20}};
// an option's place in g_options, -1: no such option
inline int option_slot(int option) {
    if (option >= 0 && option < DINT_OPT_COUNT_) return option;
    return option == DINT_OPT_QUERY_OR_PASS_PAGES ? DINT_OPT_COUNT_ : -1;
}
inline long long opt(int which) { return g_options[option_slot(which)].load(std::memory_order_relaxed); }
}  // namespace

extern "C" {

int dint_abi_version(void) { return DINT_ABI_VERSION; }

int dint_set_option(int option, long long value) {
    const int slot = option_slot(option);
    if (slot < 0) return DINT_ERR_ARG;
    if (option != DINT_OPT_QUERY_LEAN_PAGES && option != DINT_OPT_CHUNK_SPLIT && value < 0) return DINT_ERR_ARG;
    if (option == DINT_OPT_CHUNK_SPLIT && (value < -1 || value > 4)) return DINT_ERR_ARG;
    if (option == DINT_OPT_QUERY_OR_PASS_PAGES && (value < 1 || value > 0xFFFFFFFFll)) return DINT_ERR_ARG;
    g_options[slot].store(value, std::memory_order_relaxed);
    return DINT_OK;
}

int dint_get_option(int option, long long* value) {
    if (option_slot(option) < 0 || !value) return DINT_ERR_ARG;
    *value = opt(option);
    return DINT_OK;
}

const char* dint_option_name(int option) { return option_slot(option) < 0 ? nullptr : kOptionDefs[option_slot(option)].key; }

int dint_reset_options(void) {
    for (int i = 0; i != kOptionSlots; ++i) g_options[i].store(kOptionDefs[i].def, std::memory_order_relaxed);
    return DINT_OK;
}

const char* dint_strerror(int status) {
    switch (status) {
        case DINT_OK: return "ok";
        case DINT_ERR_ARG: return "bad argument";
        case DINT_ERR_FORMAT: return "malformed dictionary or stream";
        case DINT_ERR_HIP: return "HIP runtime error";
        case DINT_ERR_NO_DEVICE: return "no such device";
        case DINT_ERR_NOMEM: return "out of memory";
        default: return "unknown status";
    }
}

const char* dint_last_hip_error(void) { return g_hip_error.c_str(); }

int dint_device_count(int* count) {
    if (!count) return DINT_ERR_ARG;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *count = n;
    return DINT_OK;
}

