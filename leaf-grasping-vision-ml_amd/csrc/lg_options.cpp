// The library's reads of the environment (lg_options.h).  One line per switch: its name, its field (what the text form
// shows) and what a set variable does with its integer n (atoi: 0 for text that is no number).
#include "lg_options.h"

#include <sched.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <string>
#include <thread>

#include "lg_dt.h"

namespace {

int clamp(int v, int lo, int hi) { return std::max(lo, std::min(hi, v)); }
bool among(int v, std::initializer_list<int> set) { return std::find(set.begin(), set.end(), v) != set.end(); }

struct Parse {   // a set variable's integer goes through the switch's rule
    template <class T, class F> void operator()(const char* name, const T&, F rule) { if (const char* e = getenv(name)) rule(atoi(e)); }
};
struct Print {   // NAME=value of the field
    std::string s;
    template <class T, class F> void operator()(const char* name, const T& field, F) { s += name + ("=" + std::to_string((int)field)) + "\n"; }
};

template <class V> void each(LgOptions& o, V&& v) {
    v("LG_HOST_THREADS", o.host_threads, [&](int n) { o.host_threads = std::max(1, n); });
    v("LG_SUBBATCH", o.subbatch, [&](int n) { o.subbatch = std::max(1, n); });
    v("LG_TRACE", o.trace, [&](int) { o.trace = true; });
    v("LG_NO_SKIP", o.no_skip, [&](int n) { o.no_skip = std::max(1, n) & 3; });
    v("LG_FINAL_NEAR", o.final_near, [&](int n) { o.final_near = clamp(n, 0, 64); });
    v("LG_FINAL_PERSIST", o.final_persist, [&](int n) { o.final_persist = n; o.final_near = 0; });   // launch-shape experiments of
    v("LG_FINAL_TPW", o.final_tpw, [&](int n) { o.final_tpw = n; o.final_near = 0; });               // the full tile walk
    v("LG_HOST_ORIENT", o.host_orient, [&](int) { o.host_orient = true; });
    v("LG_CNN_PRUNE", o.cnn_prune, [&](int n) { o.cnn_prune = n != 0; });
    v("LG_DEFER_PLANES", o.defer_planes, [&](int n) { o.defer_planes = n != 0; });
    v("LG_DT_SEARCH", o.dt_search, [&](int n) { o.dt_search = clamp(n, 0, 2); });
    v("LG_DT_SEARCH_ALGO", o.dt_algo, [&](int n) { if (among(n, {0, LG_DT_FORM_ROWS, LG_DT_FORM_BANDS, LG_DT_FORM_SWEEP})) o.dt_algo = n; });
    v("LG_DT_BAND_P", o.dt_band_p, [&](int n) { if (among(n, {12, 16, 24, 32})) o.dt_band_p = n; });
    v("LG_DT_BAND_E", o.dt_band_e, [&](int n) { if (among(n, {2, 4})) o.dt_band_e = n; });
    v("LG_SIDE_TAIL", o.side_tail, [&](int n) { o.side_tail = clamp(n, 0, 2); });
    v("LG_STEM_ALGO", o.stem_algo, [&](int n) { o.stem_algo = n != 0; });
    v("LG_DIRECT_HOST", o.direct_host, [&](int n) { o.direct_host = n != 0; });
    v("LG_ORIENT_CAP", o.orient_cap, [&](int n) { o.orient_cap = clamp(n, 16, 16384); });
    v("LG_ORIENT_FAIL", o.orient_fail, [&](int) { o.orient_fail = true; });
}
template <class V> void each(LgCnnOptions& o, V&& v) {
    v("LG_CNN_F23", o.f23, [&](int) { o.f23 = true; });
    v("LG_CNN_WINO_MASK", o.wino_mask, [&](int n) { o.wino_mask = n & 0x3f; });
}
template <class V> void each(LgTrainOptions& o, V&& v) {
    v("LG_TRAIN_GRAPH", o.graph, [&](int n) { o.graph = n != 0; });
    v("LG_TRAIN_STREAMS", o.streams, [&](int n) { o.streams = n == 2 ? 2 : 1; });
    v("LG_TRAIN_CONV_SMALL", o.conv_small_below, [&](int n) { o.conv_small_below = n; });
    v("LG_TRAIN_CONV_SPLIT", o.conv_split_below, [&](int n) { o.conv_split_below = n; });
}

template <class O> int print(O o, char* buf, int cap) {
    if (!buf || cap < 1) return LG_ERR_INVALID;
    Print p;
    each(o, p);
    snprintf(buf, (size_t)cap, "%s", p.s.c_str());
    return (int)p.s.size();
}

}  // namespace

LgOptions lg_options_from_env() {
    LgOptions o;
    // host workers: this process's share of the CPUs it may run on (one process per GPU: LOCAL_WORLD_SIZE ranks split the
    // node), at most 16
    unsigned hw = std::thread::hardware_concurrency(), ranks = 1;
    cpu_set_t set;
    CPU_ZERO(&set);
    if (sched_getaffinity(0, sizeof(set), &set) == 0 && CPU_COUNT(&set) > 0) hw = (unsigned)CPU_COUNT(&set);
    if (const char* e = getenv("LOCAL_WORLD_SIZE")) ranks = (unsigned)std::max(1, atoi(e));
    o.host_threads = (int)std::max(1u, std::min((hw ? hw : 1u) / ranks, 16u));
    each(o, Parse());
    return o;
}
LgCnnOptions lg_cnn_options_from_env() {
    LgCnnOptions o;
    if (getenv("LG_CNN_DIRECT")) o.wino_mask = 0;   // (LG_CNN_WINO_MASK takes precedence)
    each(o, Parse());
    return o;
}
LgTrainOptions lg_train_options_from_env() {
    LgTrainOptions o;
    each(o, Parse());
    return o;
}

int lg_options_print(const LgOptions& o, char* buf, int cap) { return print(o, buf, cap); }
extern "C" int lg_options_text(int which, char* buf, int cap) {
    return which == 0 ? print(lg_options_from_env(), buf, cap) : which == 1 ? print(lg_cnn_options_from_env(), buf, cap)
         : which == 2 ? print(lg_train_options_from_env(), buf, cap) : LG_ERR_INVALID;
}
