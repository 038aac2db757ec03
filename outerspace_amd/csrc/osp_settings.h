// osp_settings.h -- every OSP_* environment variable the library reads: ONE table, one typed member per setting, one
// reader.  Host only, no HIP: osp_host.cpp and tests/settings_driver.cpp
// include it as plain C++.
//
// A value means what libc makes of it (atoi, atol, strtoull base 10, atof, strcmp): garbage reads 0, OSP_VERBOSE=0 is
// verbose.  An EMPTY value (OSP_X=) counts as unset for every kind but the presence flags.
//
// Defaults are not here: they live beside the constants they come from (kernel headers, device memory), so a numeric
// member says whether it was set and what was parsed, and the use site supplies the default: env.split_row_max.or_(kSplitRowMax).
#pragma once
#include <cstdint>
#include <cstdlib>
#include <string>

namespace osp {

// ---- the kinds in use ----
struct Flag {   // presence: set at all, whatever the value (OSP_GUARD also looks at the number)
    bool set = false;
    int value = 0;
    explicit operator bool() const { return set; }
    void parse(const char *v) { set = v != nullptr; value = v ? atoi(v) : 0; }
};
struct Switch {   // on unless atoi(value) == 0
    bool on = true;
    explicit operator bool() const { return on; }
    void parse(const char *v) { on = !(v && *v && atoi(v) == 0); }
};
template <class T> struct Opt {   // set or not, and the parsed value
    bool set = false;
    T value{};
    T or_(T dflt) const { return set ? value : dflt; }
};
struct Int : Opt<int> { void parse(const char *v) { if ((set = v && *v)) value = atoi(v); } };
struct Long : Opt<long> { void parse(const char *v) { if ((set = v && *v)) value = atol(v); } };
struct U64 : Opt<uint64_t> { void parse(const char *v) { if ((set = v && *v)) value = strtoull(v, nullptr, 10); } };
struct Real : Opt<double> { void parse(const char *v) { if ((set = v && *v)) value = atof(v); } };
struct Word {   // compared against fixed words
    std::string text;
    bool is(const char *w) const { return text == w; }
    void parse(const char *v) { text = v ? v : ""; }
};

// when a setting is read: by every call (the snapshot in Context::env), when a context is created, or once per process
enum When { PerCall, PerContext, PerProcess };

// ---- the table: member, name, kind, when ----
#define OSP_SETTINGS(X)                                                   \
    X(verbose, "OSP_VERBOSE", Flag, PerCall)                              \
    X(sync, "OSP_SYNC", Flag, PerProcess)                                 \
    X(poison, "OSP_POISON", Flag, PerProcess)                             \
    X(guard, "OSP_GUARD", Flag, PerProcess)                               \
    X(direct, "OSP_DIRECT", Switch, PerCall)                              \
    X(hub, "OSP_HUB", Switch, PerCall)                                    \
    X(plan_small, "OSP_PLAN_SMALL", Switch, PerCall)                      \
    X(gather_over, "OSP_GATHER_OVER", Switch, PerCall)                    \
    X(expand_rows, "OSP_EXPAND_ROWS", Switch, PerCall)                    \
    X(plan_overlap, "OSP_PLAN_OVERLAP", Switch, PerCall)                  \
    X(gather, "OSP_GATHER", Int, PerCall)                                 \
    X(split_from_b, "OSP_SPLIT_FROM_B", Int, PerCall)                     \
    X(dense_seg, "OSP_DENSE_SEG", Int, PerCall)                           \
    X(multi_subpanels, "OSP_MULTI_SUBPANELS", Int, PerCall)               \
    X(parse_threads, "OSP_PARSE_THREADS", Int, PerCall)                   \
    X(plan_small_cells, "OSP_PLAN_SMALL_CELLS", Long, PerCall)            \
    X(plan_small_chunks, "OSP_PLAN_SMALL_CHUNKS", Long, PerCall)          \
    X(direct_min_nnz, "OSP_DIRECT_MIN_NNZ", U64, PerCall)                 \
    X(direct_max, "OSP_DIRECT_MAX", U64, PerCall)                         \
    X(split_row_max, "OSP_SPLIT_ROW_MAX", U64, PerCall)                   \
    X(gather_max_runs, "OSP_GATHER_MAX_RUNS", U64, PerCall)               \
    X(bigtile_cap, "OSP_BIGTILE_CAP", U64, PerCall)                       \
    X(compact_min_waste, "OSP_COMPACT_MIN_WASTE", U64, PerCall)           \
    X(masked_heavy_min, "OSP_MASKED_HEAVY_MIN", U64, PerCall)             \
    X(masked_bucket, "OSP_MASKED_BUCKET", U64, PerCall)                   \
    X(mcl_long_min, "OSP_MCL_LONG_MIN", U64, PerCall)                     \
    X(mxm_short_cap, "OSP_MXM_SHORT_CAP", U64, PerCall)                   \
    X(mxm_batch, "OSP_MXM_BATCH", U64, PerCall)                           \
    X(mxv_group, "OSP_MXV_GROUP", U64, PerCall)                           \
    X(hub_min_share, "OSP_HUB_MIN_SHARE", Real, PerCall)                  \
    X(hub_min_run, "OSP_HUB_MIN_RUN", Real, PerCall)                      \
    X(rank, "OSP_RANK", Word, PerContext)                                 \
    X(dense_add, "OSP_DENSE_ADD", Word, PerContext)                       \
    X(transpose_path, "OSP_TRANSPOSE_PATH", Word, PerCall)                \
    X(transpose_gather, "OSP_TRANSPOSE_GATHER", Word, PerCall)            \
    X(extract_dense_map, "OSP_EXTRACT_DENSE_MAP", Word, PerCall)

struct Settings {
#define OSP_X(member, name, Kind, when) Kind member;
    OSP_SETTINGS(OSP_X)
#undef OSP_X

    // The environment as it is now.  The per-process settings are the exception: they hold what the first reader in the
    // process saw (the pool relies on OSP_GUARD / OSP_POISON / OSP_SYNC never changing under it).
    static Settings read() {
        Settings s = process();
        s.fill(false);
        return s;
    }
    static const Settings &process() {
        static const Settings once = [] { Settings s; s.fill(true); return s; }();
        return once;
    }

private:
    void fill(bool per_process) {
#define OSP_X(member, name, Kind, when) if ((when == PerProcess) == per_process) member.parse(getenv(name));
        OSP_SETTINGS(OSP_X)
#undef OSP_X
    }
};

}  // namespace osp
