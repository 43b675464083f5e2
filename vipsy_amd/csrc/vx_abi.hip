// C-ABI entry points (include/vipsy_amd.h).  Host-side launch logic only; one translation unit.
#include "vx_common.h"
#include "k_util.hip"
#include "k_mvn_enc.hip"
#include "k_mvn_enc_fast.hip"
#include "k_mvn_enc_r.hip"
#include "k_mvn_packed.hip"
#include "k_mvn_enc_bwd.hip"
#include "k_mvn_enc_bwd_fast.hip"
#include "k_irt_lik.hip"
#include "k_irt_lik_r.hip"
#include "k_irt_lik_b.hip"
#include "k_irt_lik_h.hip"
#include "k_irt1d.hip"
#include "k_irt1d_sparse.hip"
#include "k_hodina.hip"
#include "k_hodina_m.hip"
#include "k_norm_enc.hip"
#include "k_mvn_bbvi.hip"
#include "k_mvn_score.hip"
#include "k_mvn_bwd_t.hip"
#include "k_mvn_bwd_b.hip"
#include "k_mvn_fwd_b.hip"
#include "k_mvn_fwd_b2.hip"
#include "k_mvn_score_b.hip"
#include "k_mvn_bwd_hb.hip"
#include "k_mvn_bwd_hb2.hip"
#include "k_pack_fused.hip"
#include "k_fc1_bwd_c.hip"
#include "k_cdm_sf.hip"
#include "k_synth.hip"
#include "k_vaeccdm.hip"
#include "k_grid_post.hip"
#include "k_grid_counts.hip"
#include "k_grid_draw.hip"
#include "k_grid_mstep.hip"
#include "k_grid_info.hip"
#include "k_grid_pairs.hip"
#include "k_grid_fit.hip"
#include "k_grid_point.hip"
#include "k_grid_cond.hip"
#include "k_grid_counts_cond.hip"
#include "k_grid_bifactor.hip"
#include "k_grid_bifactor_counts.hip"
#include "k_sumscore.hip"
#include "k_pair_tables.hip"

#include <unordered_map>
#include <mutex>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <utility>
#include <optional>
#include <cstdio>
#include <type_traits>

namespace {

int g_num_cu = 0;
int num_cu() {
    if (g_num_cu == 0) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess)
            g_num_cu = prop.multiProcessorCount;
        if (g_num_cu <= 0) g_num_cu = 256;
    }
    return g_num_cu;
}

// the attribute is raised once per kernel and size (not per launch: nothing but launches inside a stream capture)
inline int set_lds_ptr(const void* kernel, size_t bytes) {
    if (bytes > 160 * 1024) return VX_EINVAL;
    static std::mutex mu;
    static std::unordered_map<const void*, size_t> have;
    std::lock_guard<std::mutex> lock(mu);
    auto it = have.find(kernel);
    if (it != have.end() && it->second >= bytes) return VX_OK;
    hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return (int)e;
    have[kernel] = bytes;
    return VX_OK;
}
template <typename K>
int set_lds(K kernel, size_t bytes) { return set_lds_ptr(reinterpret_cast<const void*>(kernel), bytes); }
// one launch with dynamic LDS: the attribute, the launch, its status (a kernel's defaulted arguments are passed explicitly)
template <typename K, typename... Args>
int launch_lds(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t st, Args... args) {
    const int rc = set_lds(kernel, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
    VX_CHECK_LAUNCH();
    return VX_OK;
}

inline int grid_1d(int64_t n, int block) {
    int64_t g = (n + block - 1) / block;
    const int64_t cap = (int64_t)num_cu() * 8;
    return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

inline int tril_len(int D) { return D * (D + 1) / 2; }

EncDims make_enc_dims(const vx_irt_cfg* cfg, int64_t nb) {
    EncDims dm;
    dm.D = cfg->D; dm.J = cfg->J; dm.H = cfg->H;
    dm.Hp = (cfg->H + 31) / 32 * 32;
    dm.DS = enc_ds(cfg->D);
    dm.T = tril_len(cfg->D);
    dm.nb = nb;
    return dm;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// The test seams of the library, read from the environment once (tests/test_gpu_parity.py):
//   VX_FORCE_GENERIC=1  routes everything through the shape-generic kernels (to cross-check the specialised paths);
//   VX_MFMA16           the 16-bit-MFMA kernels (fp32 operands as fp16 pairs -- f16x2, vx_common.h -- or, in the likelihood
//                       and the fc1 gradient, as bf16 terms; fp32 accumulate; results at the accuracy of the fp32-MFMA chain)
//                       are the default (unset or 1); 0 selects the fp32-MFMA kernels, f / w / h / g only the guide forward /
//                       the head weight gradient / the hidden gradient / the fc1 weight gradient on the 16-bit MFMA;
//   VX_FWD_RING=0       the large-batch guide forward pulls its head tiles per wave (the form before the shared LDS ring of
//                       k_mvn_fwd_b2.hip);
//   VX_SCORE_NO_RING    the score-function heads kernel in its plain form at every batch size.
struct Seams {
    bool generic;
    bool fwd16, w16, h16, fc1_16;                          // VX_MFMA16: f, w, h, g
    // the side streams of the guide's forward and backward (the forward's and the hidden gradient's short last rounds, the
    // fc1 and head weight gradients beside the hidden gradient) go with the fc1 seam: VX_MFMA16 = 0 / f / w / h is one stream
    bool side_streams;
    bool fwd_ring, score_ring;
};
const Seams& seams() {
    static const Seams s = [] {
        Seams v;
        const char *g = getenv("VX_FORCE_GENERIC"), *m = getenv("VX_MFMA16"), *r = getenv("VX_FWD_RING");
        v.generic = g && g[0] == '1';
        const int mode = (!m || m[0] == '1') ? 15 : (m[0] == 'f' ? 1 : m[0] == 'w' ? 2 : m[0] == 'h' ? 4 : m[0] == 'g' ? 8 : 0);
        v.fwd16 = mode & 1; v.w16 = mode & 2; v.h16 = mode & 4; v.fc1_16 = mode & 8;
        v.side_streams = v.fc1_16;
        v.fwd_ring = !(r && r[0] == '0');
        v.score_ring = getenv("VX_SCORE_NO_RING") == nullptr;
        return v;
    }();
    return s;
}
bool force_generic() { return seams().generic; }

// shapes of the packed head layout (k_pack.hip); the others keep the reference row order
bool packed_ok(const vx_irt_cfg* cfg) {
    return !force_generic() && cfg->H == 64 && cfg->J % 4 == 0 && cfg->D % 4 == 0 &&
           enc_p_lds_floats(cfg->D, cfg->J) * sizeof(float) <= 160 * 1024 &&
           enc_bwdw_fast_lds_floats(cfg->D) * sizeof(float) <= 160 * 1024;
}
// the f16x2 guide forward (k_mvn_fwd_b*.hip) and its fused pack launches (k_pack_fused.hip)
bool fwb_shape(const vx_irt_cfg* cfg) {
    return seams().fwd16 && packed_ok(cfg) && cfg->D <= 128 && fb_lds_bytes(cfg->D, cfg->J) <= 160 * 1024;
}

bool enc_cfg_ok(const vx_irt_cfg* cfg) {
    return cfg && cfg->D >= 2 && cfg->D <= 127 && cfg->H >= 1 && cfg->H <= 128 && cfg->J >= 1;
}


// ---- measurement aid (vx_prof_enable / vx_prof_read): HIP events on the launch stream around the large kernels, so
// that bench.py can price the dominant kernel against its roofline from inside the timed steps.  Off by default: the
// entry points then record nothing.
struct ProfSlot { const char* name; int64_t units; std::vector<std::pair<hipEvent_t, hipEvent_t>> ev; };
bool g_prof = false;
ProfSlot g_prof_slots[12];
int g_prof_n = 0;
struct ProfScope {
    hipEvent_t a = nullptr, b = nullptr;
    hipStream_t st;
    const char* name;
    int64_t units;                                                    // persons of this launch when it is not the whole batch (else 0)
    ProfScope(const char* nm, hipStream_t s, int64_t u = 0, bool on = true) : st(s), name(nm), units(u) {
        if (!g_prof || !on) return;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { a = nullptr; return; }
        (void)hipEventRecord(a, st);
    }
    void cancel() {                                                   // the bracket turned out not to apply: nothing is filed
        if (a) { (void)hipEventDestroy(a); a = nullptr; }
        if (b) { (void)hipEventDestroy(b); b = nullptr; }
    }
    ~ProfScope() {
        if (!a) return;
        (void)hipEventRecord(b, st);
        for (int i = 0; i < g_prof_n; ++i)
            if (!strcmp(g_prof_slots[i].name, name)) { g_prof_slots[i].units = units; g_prof_slots[i].ev.emplace_back(a, b); return; }
        if (g_prof_n < 12) {
            g_prof_slots[g_prof_n].name = name; g_prof_slots[g_prof_n].units = units;
            g_prof_slots[g_prof_n].ev.emplace_back(a, b); ++g_prof_n; return;
        }
        (void)hipEventDestroy(a); (void)hipEventDestroy(b);           // more than twelve kernel names: not recorded, not leaked
    }
};

// A second stream for work that is independent of what the launch stream does next (the fc1 weight gradient beside the head
// weight gradient of vx_mvn_enc_backward): forked and joined with events, so the caller still sees ONE ordered stream.
// One per host thread AND device: a process that drives a second GPU gets a stream of that device, not device 0's.
struct SideStream {
    hipStream_t s = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    bool init = false, ok = false;
};
SideStream& side_stream(int which, hipStream_t main_st) {
    // keyed by (host thread, device, launch stream): two call sequences that run side by side on two launch streams (the two
    // person slices of a large batch, engine.py) must not share a side stream -- they would queue behind each other there.
    // MAXMAIN launch streams a device keep a pair of side streams each; one more evicts the least recently used pair (its
    // streams and events are destroyed -- work already queued on them still completes -- so a launch stream whose handle is
    // re-used after hipStreamDestroy cannot inherit a live slot for long, and nothing aliases another live stream's pair);
    // everything is destroyed when the host thread ends.
    constexpr int MAXDEV = 16, MAXMAIN = 4;
    struct Slot { hipStream_t main_st = nullptr; SideStream ss[2]; bool used = false; uint64_t last = 0; };
    struct Slots {
        Slot s[MAXDEV][MAXMAIN];
        uint64_t clock = 0;
        static void release(Slot& sl) {
            for (SideStream& x : sl.ss) {
                if (x.s) (void)hipStreamDestroy(x.s);
                if (x.fork) (void)hipEventDestroy(x.fork);
                if (x.join) (void)hipEventDestroy(x.join);
                x = SideStream();
            }
            sl.used = false;
        }
        ~Slots() {
            for (auto& d : s) for (Slot& sl : d) if (sl.used) release(sl);
        }
    };
    static thread_local Slots slots;
    static thread_local SideStream none;                   // ok == false: the single-stream paths
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAXDEV) return none;
    Slot* sl = nullptr;
    for (int i = 0; i < MAXMAIN && !sl; ++i)
        if (slots.s[dev][i].used && slots.s[dev][i].main_st == main_st) sl = &slots.s[dev][i];
    for (int i = 0; i < MAXMAIN && !sl; ++i)
        if (!slots.s[dev][i].used) { sl = &slots.s[dev][i]; sl->used = true; sl->main_st = main_st; }
    if (!sl) {                                             // more launch streams than slots: the least recently used pair goes
        sl = &slots.s[dev][0];
        for (int i = 1; i < MAXMAIN; ++i)
            if (slots.s[dev][i].last < sl->last) sl = &slots.s[dev][i];
        Slots::release(*sl);
        sl->used = true;
        sl->main_st = main_st;
    }
    sl->last = ++slots.clock;
    SideStream& ss = sl->ss[which & 1];
    if (!ss.init) {
        ss.init = true;
        // (stream 1 carries the head weight gradient beside the launch stream's kernels.  A LOW-PRIORITY stream for it changed
        // nothing at 1M persons -- 9.58 against 9.59 ms -- and its mere existence slowed every node of a replayed graph: 1.91
        // against 1.38 ms for a 125 k-person shard)
        ss.ok = hipStreamCreateWithFlags(&ss.s, hipStreamNonBlocking) == hipSuccess &&
                hipEventCreateWithFlags(&ss.fork, hipEventDisableTiming) == hipSuccess &&
                hipEventCreateWithFlags(&ss.join, hipEventDisableTiming) == hipSuccess;
    }
    return ss;
}
// fork() orders the side stream behind the launch stream; join() orders the launch stream behind the side stream.  A scope
// that ends between the two (an error return) still joins: the caller's stream never runs ahead of side work in flight.
struct ForkScope {
    SideStream* ss = nullptr;
    hipStream_t main_st = nullptr;
    bool fork(SideStream& s, hipStream_t st) {
        if (!s.ok || hipEventRecord(s.fork, st) != hipSuccess || hipStreamWaitEvent(s.s, s.fork, 0) != hipSuccess) return false;
        ss = &s; main_st = st;
        return true;
    }
    bool active() const { return ss != nullptr; }
    hipStream_t side() const { return ss->s; }
    int join() {
        if (!ss) return VX_OK;
        SideStream* s = ss;
        ss = nullptr;
        if (hipEventRecord(s->join, s->s) != hipSuccess || hipStreamWaitEvent(main_st, s->join, 0) != hipSuccess) return VX_EINVAL;
        return VX_OK;
    }
    ~ForkScope() { (void)join(); }
};

// dm.Hp (32 / 64 / 96 / 128) as the compile-time hidden width HT = Hp / 32 of the shape-generic encoder kernels:
// f(std::integral_constant<int, HT>) launches the instance and returns the call's status
template <typename F>
int with_hidden_width(int Hp, F&& f) {
    switch (Hp) {
        case 32: return f(std::integral_constant<int, 1>());
        case 64: return f(std::integral_constant<int, 2>());
        case 96: return f(std::integral_constant<int, 3>());
        default: return f(std::integral_constant<int, 4>());
    }
}

// A short last chip round BESIDE the whole rounds (the guide forward and the hidden gradient): with a side stream whose fork
// succeeds, tail(side stream) is launched first -- its workgroups take their CUs at once, the whole rounds fill the rest, and
// they cost their share of the chip's time instead of a round of their own -- then whole() on the launch stream, then the
// join; otherwise whole(), then tail(launch stream).  The launch stream is joined on every error return too (the scope).
template <typename Tail, typename Whole>
int with_last_round(SideStream* side, hipStream_t st, Tail&& tail, Whole&& whole) {
    ForkScope fork;
    const bool beside = side && fork.fork(*side, st);
    int rc = beside ? tail(fork.side()) : whole();
    if (rc) return rc;
    rc = beside ? whole() : tail(st);
    return rc ? rc : fork.join();
}

// ---- what the entries of the grid family (vx_grid_*, vx_sumscore_*) share: an entry is a gate, a plan (grid_plan.h), a launch ----
bool hodina_cfg_ok(const vx_hodina_cfg* cfg) { return cfg && cfg->K >= 1 && cfg->K <= 10 && cfg->J >= 1 && cfg->J <= 1024; }
// The item parameters of an IRT entry: the model within 1 (1PL: D = 1, a = 1) .. max_model (2: 2PL, 3: + c_un, 4: + d_un), D within
// the entry's limit, and every array the model reads
bool irt_items_ok(const vx_irt_cfg* cfg, int max_model, int max_D, const float* a, const float* b, const float* c_un, const float* d_un) {
    if (!cfg || cfg->model < 1 || cfg->model > max_model || cfg->D < 1 || cfg->D > max_D || !b) return false;
    return !((cfg->model == 1 && cfg->D != 1) || (cfg->model >= 2 && !a) || (cfg->model >= 3 && !c_un) || (cfg->model == 4 && !d_un));
}
// The item parameters of a DINA / DINO entry
bool cdm_items_ok(const vx_hodina_cfg* cfg, int dino, const float* q, const float* g_un, const float* s_un) {
    return hodina_cfg_ok(cfg) && cfg->K <= GP_MAXD && cfg->J <= GP_MAXJ && (dino == 0 || dino == 1) && q && g_un && s_un;
}
// The draws [draw0, draw0 + ndraws) of a plausible-value entry, `stride` slots a person
bool draw_range_ok(int32_t draw0, int32_t ndraws, int64_t stride) {
    return draw0 >= 0 && draw0 <= PV_MAXDRAWS && ndraws >= 1 && ndraws <= PV_MAXDRAWS && draw0 + ndraws <= PV_MAXDRAWS &&
           (int64_t)draw0 + ndraws <= stride;
}
// cfg->model (1 .. 4, checked) as the MODEL of a kernel template: f(std::integral_constant<int, MODEL>) launches the instance
template <typename F>
int with_irt_model(int model, F&& f) {
    switch (model) {
        case 1: return f(std::integral_constant<int, 1>());
        case 2: return f(std::integral_constant<int, 2>());
        case 3: return f(std::integral_constant<int, 3>());
        default: return f(std::integral_constant<int, 4>());
    }
}
// GcPlan::it as the (IT, NTG) of k_grid_counts / k_grid_counts_cond: four item tiles a wave leave registers for one node tile only
template <typename F>
int with_counts_tiles(int it, F&& f) {
    switch (it) {
        case 1: return f(std::integral_constant<int, 1>(), std::integral_constant<int, 2>());
        case 2: return f(std::integral_constant<int, 2>(), std::integral_constant<int, 2>());
        default: return f(std::integral_constant<int, 4>(), std::integral_constant<int, 1>());
    }
}
// The tail of both expected-count entries: reduce(offset, len, out) launches the entry's sum over the chunks' slabs for each of the
// columns [n1 | n0 | mass]
template <typename Reduce>
int counts_reduce(int J, int G, float* n1, float* n0, float* mass, Reduce&& reduce) {
    const int64_t JG = (int64_t)J * G, offs[3] = {0, JG, 2 * JG}, lens[3] = {JG, JG, (int64_t)G};
    float* const outs[3] = {n1, n0, mass};
    for (int k = 0; k < 3; ++k) {
        reduce(offs[k], lens[k], outs[k]);
        VX_CHECK_LAUNCH();
    }
    return VX_OK;
}
// The slab loop of vx_grid_info and vx_grid_pairs_* (SlabPlan, grid_plan.h).  For each slab of persons [i0, i0 + ns): frag(i0, ns)
// launches the entry's fragment kernel into the head of the workspace and returns the 32-person units it wrote; `xprod` (the
// cross products of those units, `xthreads` a workgroup) leaves a set of partial tiles a chunk; the chunks are added in ascending
// order, the slabs in person order.  finish() launches what turns the running sum into the entry's outputs.
using SlabXprod = void (*)(const uint4*, int, int, int64_t, int64_t, float*, int64_t);
template <typename Frag, typename Finish>
int grid_slab_loop(const SlabPlan& p, int64_t nb, float* workspace, void* hs, SlabXprod xprod, int xthreads, Frag&& frag,
                   Finish&& finish) {
    hipStream_t st = (hipStream_t)hs;
    float *part = workspace + p.off_part, *red = workspace + p.off_red, *acc = workspace + p.off_acc;
    for (int64_t i0 = 0; i0 < nb; i0 += p.slab_persons) {
        const int64_t ns = nb - i0 < p.slab_persons ? nb - i0 : p.slab_persons;
        const int64_t n_units = frag(i0, ns);
        VX_CHECK_LAUNCH();
        hipLaunchKernelGGL(xprod, dim3((unsigned)(p.n_bp * p.n_chunks)), dim3(xthreads), 0, st, (const uint4*)workspace, p.tiles, p.nbb,
                           n_units, p.units_per_chunk, part, p.tiles_len);
        VX_CHECK_LAUNCH();
        const int rc = vx_reduce_slabs(part, p.n_chunks, p.tiles_len, 1.0f, red, hs);
        if (rc) return rc;
        hipLaunchKernelGGL(k_info_add, dim3(grid_1d(p.tiles_len, 256)), dim3(256), 0, st, acc, (const float*)red, p.tiles_len,
                           i0 == 0 ? 1 : 0);
        VX_CHECK_LAUNCH();
    }
    finish();
    VX_CHECK_LAUNCH();
    return VX_OK;
}
// vx_grid_pairs_irt / vx_grid_pairs_cdm on that loop: launch(i0, ns, n_units, grid) launches the entry's cell kernel (k_pair_frag*)
// over the n_units = ceil(ns / 32) units of a slab
template <typename Launch>
int grid_pairs_run(int64_t nb, int J, float* n, float* s, float* ss, float* sp, float* workspace, int64_t ws_floats, void* hs,
                   Launch&& launch) {
    const SlabPlan p = pp_slab_plan(nb, J, ws_floats);
    auto frag = [&](int64_t i0, int64_t ns) -> int64_t {
        const int64_t n_units = (ns + 31) / 32, cap = (int64_t)num_cu() * 8;
        launch(i0, ns, n_units, dim3((unsigned)(n_units < cap ? n_units : cap)));
        return n_units;
    };
    return grid_slab_loop(p, nb, workspace, hs, k_pair_xprod, 64 * PP_XWAVES, frag, [&] {
        hipLaunchKernelGGL(k_pair_finish, dim3(grid_1d((int64_t)J * J, 256)), dim3(256), 0, (hipStream_t)hs,
                           (const float*)(workspace + p.off_acc), J, p.tiles, n, s, ss, sp);
    });
}
}  // namespace

extern "C" {

int vx_abi_version(void) { return VX_ABI_VERSION; }
const char* vx_build_info(void) { return "vipsy_amd gfx950 fp32-mfma " __DATE__ " " __TIME__; }

int vx_prof_enable(int on) {
    if (on == 2 || on == 3) { g_prof = on == 2; return VX_OK; }       // resume / pause: the records stay
    for (int i = 0; i < g_prof_n; ++i) {
        for (auto& e : g_prof_slots[i].ev) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
        g_prof_slots[i].ev.clear();
    }
    g_prof_n = 0;
    g_prof = on != 0;
    return VX_OK;
}

int vx_prof_count(void) { return g_prof_n; }

int vx_prof_read(int slot, char* name, int name_cap, float* mean_ms, int* launches) {
    if (slot < 0 || slot >= g_prof_n || !name || name_cap < 1 || !mean_ms || !launches) return VX_EINVAL;
    const ProfSlot& s = g_prof_slots[slot];
    strncpy(name, s.name, (size_t)name_cap - 1);
    name[name_cap - 1] = 0;
    double tot = 0;
    for (auto& e : s.ev) {
        float ms = 0.f;
        if (hipEventSynchronize(e.second) != hipSuccess || hipEventElapsedTime(&ms, e.first, e.second) != hipSuccess)
            return VX_EINVAL;
        tot += ms;
    }
    *launches = (int)s.ev.size();
    *mean_ms = s.ev.empty() ? 0.f : (float)(tot / s.ev.size());
    return VX_OK;
}

int vx_prof_units(int slot, int64_t* units) {
    if (slot < 0 || slot >= g_prof_n || !units) return VX_EINVAL;
    *units = g_prof_slots[slot].units;
    return VX_OK;
}

int vx_philox_normals(float* eps, const int64_t* gids, int64_t gid0, int64_t n, int32_t D, uint64_t seed,
                      uint32_t step, uint32_t stream, void* hs) {
    if (!eps || n < 0 || D < 1) return VX_EINVAL;
    if (n == 0) return VX_OK;
    const int64_t total = n * ((D + 3) / 4);
    hipLaunchKernelGGL(k_philox_normals, dim3(grid_1d(total, 256)), dim3(256), 0, (hipStream_t)hs, eps, gids,
                       gid0, n, (int)D, seed, step, stream);
    VX_CHECK_LAUNCH();
    return VX_OK;
}

int vx_philox_raw(uint32_t* out, int64_t gid0, int64_t n, uint64_t seed, uint32_t step, uint32_t stream,
                  void* hs) {
    if (!out || n < 0) return VX_EINVAL;
    if (n == 0) return VX_OK;
    hipLaunchKernelGGL(k_philox_raw, dim3(grid_1d(n, 256)), dim3(256), 0, (hipStream_t)hs, out, gid0, n, seed,
                       step, stream);
    VX_CHECK_LAUNCH();
    return VX_OK;
}

int vx_reduce_slabs(const float* slabs, int64_t n_slabs, int64_t len, float alpha, float* out, void* hs) {
    if (!slabs || !out || n_slabs < 1 || len < 0) return VX_EINVAL;
    if (len == 0) return VX_OK;
    if (n_slabs <= 8 && len >= (1 << 16) && len % 4 == 0 && aligned16(slabs) && aligned16(out)) {
        hipLaunchKernelGGL(k_reduce_few, dim3(num_cu() * 8), dim3(256), 0, (hipStream_t)hs, (const float4*)slabs,
                           (int)n_slabs, len / 4, len / 4, alpha, (float4*)out);
        VX_CHECK_LAUNCH();
        return VX_OK;
    }
    hipLaunchKernelGGL(k_reduce_slabs, dim3(grid_1d(len, 64)), dim3(256), 0, (hipStream_t)hs, slabs, n_slabs,
                       len, len, alpha, out);
    VX_CHECK_LAUNCH();
    return VX_OK;
}

// the tail of a D = 1 step: slabs of [4 J item gradients | ELBO share] -> gitem, loss; the device step counter advances.
// opt (vx_irt1d_grad_adam): the optimiser in the same launch (k_reduce_adam)
static int reduce_step_slabs(const float* slabs, int64_t n_slabs, int J, float* gitem, float* loss, uint32_t* tick,
                             void* hs, const vx_adam_tail* opt = nullptr) {
    const int64_t len = 4 * (int64_t)J + (loss ? 1 : 0);
    if (opt) {
        if (!loss || !opt->pA || !opt->mA || !opt->vA || !opt->segsA || opt->nA != 4 * (int64_t)J || opt->n_segsA < 1 ||
            opt->n_segsA > VX_MAX_SEGS || opt->nB < 0 || opt->n_segsB < 0 || opt->n_segsB > VX_MAX_SEGS ||
            (opt->nB > 0 && (!opt->pB || !opt->gB || !opt->mB || !opt->vB || !opt->segsB || opt->n_segsB < 1)) ||
            (opt->t < 1 && !tick))
            return VX_EINVAL;
        AdamSegs sa, sb;
        sa.n = opt->n_segsA; sb.n = opt->nB > 0 ? opt->n_segsB : 0;
        for (int i = 0; i < sa.n; ++i) {
            if (opt->segsA[i].begin < 0 || opt->segsA[i].end > opt->nA || opt->segsA[i].begin > opt->segsA[i].end) return VX_EINVAL;
            sa.begin[i] = opt->segsA[i].begin; sa.end[i] = opt->segsA[i].end; sa.lr[i] = opt->segsA[i].lr;
        }
        for (int i = 0; i < sb.n; ++i) {
            if (opt->segsB[i].begin < 0 || opt->segsB[i].end > opt->nB || opt->segsB[i].begin > opt->segsB[i].end) return VX_EINVAL;
            sb.begin[i] = opt->segsB[i].begin; sb.end[i] = opt->segsB[i].end; sb.lr[i] = opt->segsB[i].lr;
        }
        const AdamBuf A{opt->pA, gitem, opt->mA, opt->vA, opt->freeA, opt->nA}, B{opt->pB, opt->gB, opt->mB, opt->vB, nullptr, opt->nB};
        const double bc1 = 1.0 - pow((double)opt->beta1, (double)(tick ? 1 : opt->t));
        const double bc2 = 1.0 - pow((double)opt->beta2, (double)(tick ? 1 : opt->t));
        // Adam's count of a captured step: the word the step kernel left behind its slabs (one slab = 4 J + 1 floats)
        const uint32_t* t_copy = tick ? (const uint32_t*)(slabs + n_slabs * (4 * (int64_t)J + 1)) : nullptr;
        int64_t nb_blk = ((opt->nB + 3) / 4 + 1023) / 1024;                      // four elements a thread (adam_quad)
        if (nb_blk > (int64_t)num_cu() * 2) nb_blk = (int64_t)num_cu() * 2;
        if (n_slabs > 512) {
            const int n_red = grid_1d(len, 8);
            hipLaunchKernelGGL(k_reduce_adam<8>, dim3((unsigned)(n_red + nb_blk)), dim3(1024), 0, (hipStream_t)hs, slabs, n_slabs,
                               4 * (int64_t)J + 1, len, -1.0f, gitem, loss, tick, t_copy, (uint32_t)opt->t, A, sa, B, sb, opt->beta1,
                               opt->beta2, opt->eps, (float)bc1, (float)sqrt(bc2), opt->loss_ring, n_red);
        } else {
            const int n_red = grid_1d(len, 32);
            hipLaunchKernelGGL(k_reduce_adam<32>, dim3((unsigned)(n_red + nb_blk)), dim3(1024), 0, (hipStream_t)hs, slabs, n_slabs,
                               4 * (int64_t)J + 1, len, -1.0f, gitem, loss, tick, t_copy, (uint32_t)opt->t, A, sa, B, sb, opt->beta1,
                               opt->beta2, opt->eps, (float)bc1, (float)sqrt(bc2), opt->loss_ring, n_red);
        }
        VX_CHECK_LAUNCH();
        return VX_OK;
    }
    if (n_slabs > 512)
        hipLaunchKernelGGL(k_reduce_wide<8>, dim3(grid_1d(len, 8)), dim3(1024), 0, (hipStream_t)hs, slabs, n_slabs,
                           4 * (int64_t)J + 1, len, -1.0f, gitem, loss, tick);
    else
        hipLaunchKernelGGL(k_reduce_wide<32>, dim3(grid_1d(len, 32)), dim3(1024), 0, (hipStream_t)hs, slabs, n_slabs,
                           4 * (int64_t)J + 1, len, -1.0f, gitem, loss, tick);
    VX_CHECK_LAUNCH();
    return VX_OK;
}

int64_t vx_sum_workspace_floats(void) { return 1024; }

// the sum of v1 (+ v2, when given) in one launch (a small batch: k_sum_stage1's final form) or two
static int sum_impl(const float* v1, const float* v2, int64_t n, float alpha, float* out, float* workspace, uint32_t* step_dev, void* hs) {
    int nblk = (int)((n + 4095) / 4096);
    if (nblk < 1) nblk = 1;
    if (nblk > 1024) nblk = 1024;
    if (nblk == 1) {
        hipLaunchKernelGGL(k_sum_stage1, dim3(1), dim3(256), 0, (hipStream_t)hs, v1, n, workspace, v2, alpha, out, step_dev);
        VX_CHECK_LAUNCH();
        return VX_OK;
    }
    hipLaunchKernelGGL(k_sum_stage1, dim3(nblk), dim3(256), 0, (hipStream_t)hs, v1, n, workspace, v2);
    VX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_sum_stage2, dim3(1), dim3(256), 0, (hipStream_t)hs, workspace, nblk, alpha, out, step_dev);
    VX_CHECK_LAUNCH();
    return VX_OK;
}

int vx_sum(const float* v, int64_t n, float alpha, float* out, float* workspace, uint32_t* step_dev, void* hs) {
    if (!v || !out || !workspace || n < 0) return VX_EINVAL;
    return sum_impl(v, nullptr, n, alpha, out, workspace, step_dev, hs);
}

int vx_sum2(const float* v1, const float* v2, int64_t n, float alpha, float* out, float* workspace, uint32_t* step_dev, void* hs) {
    if (!v1 || !v2 || !out || !workspace || n < 0) return VX_EINVAL;
    return sum_impl(v1, v2, n, alpha, out, workspace, step_dev, hs);
}

int vx_adam_step(float* p, const float* g, float* m, float* v, const float* free_mask, int64_t n,
                 const vx_adam_seg* segs, int32_t n_segs, int32_t t, const uint32_t* t_dev, float beta1, float beta2,
                 float eps, const float* loss_src, float* loss_ring, void* hs) {
    if (!p || !g || !m || !v || !segs || n_segs < 1 || n_segs > VX_MAX_SEGS || (t < 1 && !t_dev) || (loss_ring && !loss_src))
        return VX_EINVAL;
    AdamSegs s;
    s.n = n_segs;
    for (int i = 0; i < n_segs; ++i) {
        if (segs[i].begin < 0 || segs[i].end > n || segs[i].begin > segs[i].end) return VX_EINVAL;
        s.begin[i] = segs[i].begin; s.end[i] = segs[i].end; s.lr[i] = segs[i].lr;
    }
    const double bc1 = 1.0 - pow((double)beta1, (double)(t_dev ? 1 : t));
    const double bc2 = 1.0 - pow((double)beta2, (double)(t_dev ? 1 : t));
    hipLaunchKernelGGL(k_adam, dim3(grid_1d((n + 3) / 4, 256)), dim3(256), 0, (hipStream_t)hs, p, g, m, v, free_mask, n, s,
                       beta1, beta2, eps, (float)bc1, (float)sqrt(bc2), t_dev, (uint32_t)t, loss_src, loss_ring);
    VX_CHECK_LAUNCH();
    return VX_OK;
}

int vx_adam_step2(float* pA, const float* gA, float* mA, float* vA, const float* freeA, int64_t nA, const vx_adam_seg* segsA,
                  int32_t n_segsA, float* pB, const float* gB, float* mB, float* vB, int64_t nB, const vx_adam_seg* segsB,
                  int32_t n_segsB, int32_t t, const uint32_t* t_dev, float beta1, float beta2, float eps, const float* loss_src,
                  float* loss_ring, void* hs) {
    if (!pA || !gA || !mA || !vA || !segsA || !pB || !gB || !mB || !vB || !segsB || n_segsA < 1 || n_segsA > VX_MAX_SEGS ||
        n_segsB < 1 || n_segsB > VX_MAX_SEGS || nA < 0 || nB < 0 || (t < 1 && !t_dev) || (loss_ring && !loss_src))
        return VX_EINVAL;
    AdamSegs sa, sb;
    sa.n = n_segsA; sb.n = n_segsB;
    for (int i = 0; i < n_segsA; ++i) {
        if (segsA[i].begin < 0 || segsA[i].end > nA || segsA[i].begin > segsA[i].end) return VX_EINVAL;
        sa.begin[i] = segsA[i].begin; sa.end[i] = segsA[i].end; sa.lr[i] = segsA[i].lr;
    }
    for (int i = 0; i < n_segsB; ++i) {
        if (segsB[i].begin < 0 || segsB[i].end > nB || segsB[i].begin > segsB[i].end) return VX_EINVAL;
        sb.begin[i] = segsB[i].begin; sb.end[i] = segsB[i].end; sb.lr[i] = segsB[i].lr;
    }
    const AdamBuf A{pA, gA, mA, vA, freeA, nA}, B{pB, gB, mB, vB, nullptr, nB};
    const double bc1 = 1.0 - pow((double)beta1, (double)(t_dev ? 1 : t));
    const double bc2 = 1.0 - pow((double)beta2, (double)(t_dev ? 1 : t));
    hipLaunchKernelGGL(k_adam2, dim3(grid_1d((nA + 3) / 4 + (nB + 3) / 4, 256)), dim3(256), 0, (hipStream_t)hs, A, sa, B, sb, beta1, beta2, eps,
                       (float)bc1, (float)sqrt(bc2), t_dev, (uint32_t)t, loss_src, loss_ring);
    VX_CHECK_LAUNCH();
    return VX_OK;
}

// ------------------------------------------------------------------------------------------------
// the f16x2 likelihood kernel (k_irt_lik_h.hip): D + 1 in (96, 112], 1PL / 2PL link
static bool lik_h_shape(const vx_irt_cfg* cfg) {
    return !force_generic() && cfg->D >= 96 && cfg->D <= 16 * LB_NKS - 1 && cfg->model <= VX_IRT_2PL;
}
// bytes of its x image's 64-person tiles: the overflow word stands behind them (vx_irt_lik_ximg_bytes)
static int64_t lik_ximg_ovf_bytes(int64_t nb) { return (nb + LB_P - 1) / LB_P * (int64_t)LH_XT_BYTES; }

// person slices of a grid of `groups` slab groups: as many as fill the chip once (at least one, at most the person tiles)
static int spread(int64_t n_ptiles, int64_t groups) {
    int64_t w = num_cu() / groups;
    if (w < 1) w = 1;
    return (int)(n_ptiles < 1 ? 1 : (n_ptiles < w ? n_ptiles : w));
}

// The pack buffer of the guide (vx_mvn_pack_floats), float offsets:
//   Wp | bp | gtab | WpT | f16x2 tile images of the heads (gt2: their OFF group table) | f16x2 k-step images of fc1 | f16x2
//   unit images of the hidden gradient | the operands' powers of two (sc; hscale: hT's, maxw: the words that collect the
//   step's operand maxima)
struct PackLayout { int64_t Rp, bp, gtab, wpT, img, gt2, w1img, himg, sc, hscale, maxw, total; };
static PackLayout pack_layout(const vx_irt_cfg* cfg) {
    static_assert(FB_IMG_BYTES % 4 == 0, "the tile images fill whole floats");
    PackLayout l;
    l.Rp = pk_rows(cfg->D);
    l.bp = l.Rp * 64;                      // (Wp at 0)
    l.gtab = l.bp + l.Rp;
    l.wpT = l.gtab + l.Rp / 8 + 8;
    l.img = l.wpT + l.Rp * 64;
    l.gt2 = l.img + (int64_t)fb_tiles(cfg->D) * (FB_IMG_BYTES / 4);
    l.w1img = l.img + fb_img_floats(cfg->D);
    l.himg = l.w1img + fb_w1img_floats(cfg->J);
    l.sc = l.himg + hb_img_floats(cfg->D);
    l.hscale = l.sc + 3;
    l.maxw = l.sc + 11;
    l.total = l.sc + FB_NSCALES;
    return l;
}

// The plan of the guide's forward and backward calls for (cfg, nb): the kernels the shape allows, the grids and the layout of
// the backward's workspace (vx_mvn_enc_bwd_workspace_floats).  Which kernels a call launches also depends on its pointers
// (alignment, the optional buffers it passes, the gd_ready bits): bwd_route() resolves that into a BwdRoute before the first
// launch; the layout depends on (cfg, nb) and the seams alone, as the size and offset queries do.  Workspace, float offsets:
//   ghpre [nb][H] | weight-gradient slabs [n_prw_ws][lenw] | fc1 slabs [n_prf][lenf] | gdT [D][nb] + 4 | hs: two fp16 copies of
//   hT [nb][64] | unit images of the hidden gradient | the step's operand maxima [8]
// gdT exists with the dimension-major kernels (bwt), hs with the bf16 head weight gradient (bwb), the unit images with the
// f16x2 hidden gradient (bwhb); the offsets of absent regions are -1.
struct MvnPlan {
    bool packed;                 // the packed head layout (k_pack.hip)
    bool fwb;                    // the f16x2 forward (k_mvn_fwd_b*.hip) and its fused pack launches
    bool encb_fast;              // the person-major backward's fast kernels (k_mvn_enc_bwd_fast.hip)
    bool bwt;                    // the dimension-major weight gradient (k_mvn_bwd_t.hip)
    bool bwh_t;                  // ... and hidden gradient: vx_mvn_enc_bwd_layout == 1, the backward reads gxT only
    bool bwb;                    // the head weight gradient on the bf16 MFMA (k_mvn_bwd_b.hip)
    bool bwhb;                   // the hidden gradient on the f16x2 MFMA (k_mvn_bwd_hb*.hip)
    bool hb_fw;                  // fwb && bwhb: the unit images and the operand maxima in packws (k_pack_fused.hip)
    bool fc1_16, side_streams;   // the seams (Seams)
    int n_rowslabs, n_prw;       // the person-major weight gradient's grid
    int n_rowslabs_t, n_prw_t;   // the dimension-major weight gradient's grid
    int n_jg, n_prf;             // the fc1 gradient's grid
    int n_prw_ws;                // weight-gradient slabs in the workspace: either of the two grids fits
    int64_t lenw_ref, lenw, lenf;
    int64_t slabs_w, slabs_f, gd = -1, hs = -1, himg = -1, maxw, total;
};
static MvnPlan mvn_plan(const vx_irt_cfg* cfg, int64_t nb) {
    const Seams& sm = seams();
    const int64_t D = cfg->D, J = cfg->J, H = cfg->H, T = tril_len(cfg->D), Rp = pk_rows(cfg->D);
    MvnPlan p;
    p.packed = packed_ok(cfg);
    p.fwb = fwb_shape(cfg);
    p.encb_fast = !sm.generic && H == 64 && D % 4 == 0 && enc_bwdw_fast_lds_floats(cfg->D) * sizeof(float) <= 160 * 1024;
    p.bwt = p.packed && nb % 4 == 0 && D <= 124 && bt_lds_bytes(cfg->D) <= 160 * 1024;
    p.bwh_t = p.bwt && nb >= 4 && bh_lds_bytes(cfg->D) <= 160 * 1024;
    p.bwb = sm.w16 && p.bwt && nb % 8 == 0 && nb < ((int64_t)1 << 23) && bb_lds_bytes(cfg->D) <= 160 * 1024;
    p.bwhb = sm.h16 && p.bwt && nb >= 4 && D <= 16 * HB_NS && hb_lds_bytes(cfg->D) <= 160 * 1024;
    p.hb_fw = p.fwb && p.bwhb;
    p.fc1_16 = sm.fc1_16;
    p.side_streams = sm.side_streams;
    const int rows_per_wg = p.encb_fast ? BWF_ROWS : BW_ROWS;
    p.n_rowslabs = (int)(((p.packed ? Rp : T + D) + rows_per_wg - 1) / rows_per_wg);
    p.n_jg = (int)((J + FC1_JG - 1) / FC1_JG);
    const int64_t n_ptiles = (nb + ENC_P - 1) / ENC_P;
    p.n_prw = spread(n_ptiles, p.n_rowslabs);
    p.n_prf = spread(n_ptiles, p.n_jg);
    p.n_rowslabs_t = (int)((Rp + BT_ROWS - 1) / BT_ROWS);
    p.n_prw_t = spread((nb + BT_P - 1) / BT_P, p.n_rowslabs_t);
    p.n_prw_ws = (p.bwt && p.n_prw_t > p.n_prw) ? p.n_prw_t : p.n_prw;
    p.lenw_ref = D * H + D + T * H + T;
    p.lenw = (p.packed && Rp * (H + 1) > p.lenw_ref) ? Rp * (H + 1) : p.lenw_ref;
    p.lenf = H * J + H;
    p.slabs_w = nb * H;
    p.slabs_f = p.slabs_w + p.n_prw_ws * p.lenw;
    int64_t end = p.slabs_f + p.n_prf * p.lenf;
    if (p.bwt) { p.gd = end; end += nb * D + 4; }
    if (p.bwb) { p.hs = end; end += nb * 64; }
    if (p.bwhb) { p.himg = end; end += hb_img_floats(cfg->D); }
    p.maxw = end;
    p.total = end + 8;
    return p;
}

// fc1's weight gradient from person-major operands with 16-byte loads (k_fc1_bwd)
static int f1fast_ok(const vx_irt_cfg* cfg, const float* ghpre, const uint8_t* y) {
    return (!force_generic() && cfg->H == 64 && cfg->J % 4 == 0 && aligned16(ghpre) && aligned16(y)) ? 1 : 0;
}

// fc1's weight gradient from person-major operands (k_fc1_bwd): slabs_f[n_prf][lenf].  A small batch (the reference's
// B = 100: two person tiles) takes 128 items a workgroup instead of 512 -- four times the workgroups, a quarter of the MFMA
// chain, the response words and the slab piece each
static bool fc1_small_batch(int Hp, int n_jg, int n_prf) { return Hp == 64 && (int64_t)n_jg * n_prf * 16 <= num_cu(); }
static int fc1_bwd_person_major(const EncDims& dm, bool small, int n_jg, int n_prf, const uint8_t* y, const int64_t* rows,
                                const float* ghpre, float* slabs_f, int64_t lenf, int f1fast, hipStream_t st) {
    const size_t lds = fc1_bwd_lds_floats(dm.Hp) * sizeof(float);
    if (small)
        return launch_lds(k_fc1_bwd<2, 1>, dim3((unsigned)((dm.J + 127) / 128), (unsigned)n_prf), dim3(ENC_THREADS), lds, st, dm, y, rows,
                          ghpre, slabs_f, lenf, f1fast);
    return with_hidden_width(dm.Hp, [&](auto ht) -> int {
        return launch_lds(k_fc1_bwd<decltype(ht)::value>, dim3((unsigned)n_jg, (unsigned)n_prf), dim3(ENC_THREADS), lds, st, dm, y, rows,
                          ghpre, slabs_f, lenf, f1fast);
    });
}

// One call of the guide's forward: the entry point's arguments, the plan and what the entry point derived from them
// (packed: the packed path is usable; ring: the step's row indices, left in the pinned host ring for the fused pack only).
extern "C++" struct FwdCall {                               // (C++ linkage: it has a member template)
    const vx_irt_cfg* cfg; MvnPlan p; EncDims dm; bool packed;
    const uint8_t* y; const int64_t* rows; int64_t nb, gid0;
    const float *W1, *b1, *W21, *b21, *W22, *b22, *eps_in;
    float *h, *x, *eps, *ldT, *ent, *hT, *epsT, *packws;
    uint8_t* ximg; uint16_t* hs_out; hipStream_t st; const int64_t* ring;
    // one launch of an f16x2 forward kernel (k_mvn_fwd_b*.hip) on the images of fwd_pack_fused; more: the first person of a
    // launch that is not the whole batch
    template <typename K, typename... More>
    int launch_b(K kernel, unsigned grid, unsigned threads, size_t lds, hipStream_t s, More... more) const {
        const PackLayout pk = pack_layout(cfg);
        return launch_lds(kernel, dim3(grid), dim3(threads), lds, s, dm, y, rows, gid0, (const uint8_t*)(packws + pk.w1img), b1,
                          (const uint8_t*)(packws + pk.img), (const uint32_t*)(packws + pk.gt2), (const float*)(packws + pk.sc), eps_in,
                          cfg->seed, cfg->step, cfg->step_dev, cfg->stream, h, x, eps, ldT, ent, hT, epsT, ximg, hs_out, more...);
    }
};

// the packed copy of the heads and the powers of two of the f16x2 operands (the backward kernels read them too), for the
// packed fp32 forward
static int fwd_pack_heads(const FwdCall& c) {
    const PackLayout pk = pack_layout(c.cfg);
    float* sc = c.packws + pk.sc;
    hipLaunchKernelGGL(k_pack_heads, dim3((unsigned)pk.Rp), dim3(64), 0, c.st, (int)c.cfg->D, 64, c.W21, c.b21, c.W22, c.b22,
                       c.packws, c.packws + pk.bp, (uint32_t*)(c.packws + pk.gtab), c.packws + pk.wpT);
    VX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_clear_words, dim3(1), dim3(64), 0, c.st, (uint32_t*)(c.packws + pk.maxw), 4);
    hipLaunchKernelGGL(k_enc_scales_max, dim3(FB_SC_BLOCKS), dim3(256), 0, c.st, (int)c.dm.D, (int)c.dm.J, c.W1, c.b1, c.W21,
                       c.b21, c.W22, c.b22, sc);
    hipLaunchKernelGGL(k_enc_scales, dim3(1), dim3(64), 0, c.st, sc);
    VX_CHECK_LAUNCH();
    return VX_OK;
}

// every weight image of the step in two launches (k_pack_fused.hip), for the f16x2 forward.  The unit images of the hidden
// gradient are made here too when that kernel will run (p.hb_fw: the backward call then reads them from packws), and WpT
// only when a kernel of this step reads it (the fp32 hidden-gradient kernel)
static int fwd_pack_fused(const FwdCall& c) {
    const PackLayout pk = pack_layout(c.cfg);
    const EncDims& dm = c.dm;
    float *Wp = c.packws, *bp = c.packws + pk.bp, *sc = c.packws + pk.sc;
    uint32_t* gtab = (uint32_t*)(c.packws + pk.gtab);
    const int n_tiles = fb_tiles(dm.D);
    // with the f16x2 hidden gradient (hb) no kernel of the step reads the packed copy Wp / bp / WpT: stage 1 is the maxima
    // alone and stage 2 takes the tile images from the parameters themselves (direct; and writes gtab, which the head weight
    // gradient reads)
    const bool hb = c.p.hb_fw, direct = hb;
    uint8_t* himg = hb ? (uint8_t*)(c.packws + pk.himg) : nullptr;
    const int n_row_blocks = direct ? 0 : (int)((pk.Rp + 3) / 4), n_w1 = (dm.J + 15) / 16;
    hipLaunchKernelGGL(k_pack_stage1, dim3(n_row_blocks + FB_SC_BLOCKS + (c.ring ? 1 : 0)), dim3(256), 0, c.st,
                       (int)dm.D, (int)dm.J, c.W1, c.b1, c.W21, c.b21, c.W22, c.b22, Wp, bp, gtab, hb ? (float*)nullptr : c.packws + pk.wpT,
                       sc, c.ring, (int64_t)c.cfg->rows_ring_stride, (int)c.cfg->rows_ring_slots, c.cfg->step_dev,
                       const_cast<int64_t*>(c.rows), c.nb, n_row_blocks);
    VX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_pack_stage2, dim3(n_w1 + n_tiles + (hb ? hb_units(dm.D) : 0)), dim3(256), 0, c.st,
                       (int)dm.D, (int)dm.J, n_tiles, pk_off_total(dm.D) / 8, c.W1, c.W21, c.W22, (const float*)Wp, (const float*)bp,
                       (const uint32_t*)gtab, sc, (uint8_t*)(c.packws + pk.w1img), (uint8_t*)(c.packws + pk.img),
                       (uint32_t*)(c.packws + pk.gt2), himg, direct ? c.b21 : (const float*)nullptr,
                       direct ? c.b22 : (const float*)nullptr, direct ? gtab : (uint32_t*)nullptr);
    VX_CHECK_LAUNCH();
    return VX_OK;
}

// packed f16x2, small batch: one 32-person tile per workgroup, its four waves share the head tiles
static int fwd_b_small(const FwdCall& c) {
    ProfScope ps("k_mvn_enc_fwd_b", c.st);
    // (with an x image: whole 64-person tiles, the absent half gets its zero rows)
    const unsigned gs = c.ximg ? (unsigned)(((c.nb + 63) / 64) * 2) : (unsigned)((c.nb + FB_WP - 1) / FB_WP);
    return c.launch_b(k_mvn_enc_fwd_b<true>, gs, FB_THREADS, fb_lds_bytes(c.dm.D, c.dm.J), c.st, (int64_t)0);
}

// packed f16x2, large batch: k_mvn_fwd_b2.hip with ONE person set per wave -- 128-person workgroups, two of them on a CU (two
// waves per SIMD, out of step): 2.74 against 2.86-2.97 ms for the 64-persons-per-wave form on the same box
// (tools/fwd2_bench.hip).  A chip round is 65 536 persons either way: a last round that fills less than half the chip goes
// to the 128-person kernel of k_mvn_fwd_b.hip (1M persons: 15 full rounds + 16 960 persons), beside the whole rounds
static int fwd_b_large(const FwdCall& c) {
    const EncDims& dm = c.dm;
    const int64_t nb = c.nb;
    const size_t ldsb = fb_lds_bytes(dm.D, dm.J);
    constexpr int FNS = 1;
    int64_t n_done = 0;                                     // persons taken by k_mvn_enc_fwd_b2
    if (fb2_lds_bytes(dm.D, dm.J, FNS) <= 80 * 1024) {
        const int64_t round2 = (int64_t)FB2_WAVES * 64 * num_cu();
        const int64_t rem = nb % round2;
        n_done = (rem > 0 && 2 * rem <= round2) ? nb - rem : nb;
        n_done -= n_done % (FB2_WAVES * 64);            // whole 64-person tiles of the x image, whole workgroups
    }
    auto last_round = [&](hipStream_t ts) -> int {
        // (timed only when it runs alone: beside the whole rounds its bracket spans theirs)
        ProfScope ps("k_mvn_enc_fwd_b", ts, nb - n_done, ts == c.st);
        return c.launch_b(k_mvn_enc_fwd_b<false>, (unsigned)((nb - n_done + FB_WAVES * FB_WP - 1) / (FB_WAVES * FB_WP)), FB_THREADS,
                          ldsb, ts, n_done);
    };
    auto whole_rounds = [&]() -> int {
        // the head tiles through the workgroup's LDS ring where the shape allows it: a quarter of the L2 -> CU bytes
        const bool tile_ring = seams().fwd_ring && fb2s_shape_ok((int)dm.D, (int)dm.J);
        const size_t lds2 = tile_ring ? fb2s_lds_bytes((int)dm.D) : fb2_lds_bytes(dm.D, dm.J, FNS);
        ProfScope ps("k_mvn_enc_fwd_b2", c.st, n_done);
        const int wg = FB2_WAVES * 32 * FNS;
        const unsigned grid2 = (unsigned)((n_done + wg - 1) / wg);                                          // the grid stops at n_done
        return tile_ring ? c.launch_b(k_mvn_enc_fwd_b2<FNS, true>, grid2, FB2_THREADS, lds2, c.st)
                         : c.launch_b(k_mvn_enc_fwd_b2<FNS, false>, grid2, FB2_THREADS, lds2, c.st);
    };
    if (n_done == 0) return last_round(c.st);
    if (n_done == nb) return whole_rounds();
    return with_last_round(c.p.side_streams ? &side_stream(0, c.st) : nullptr, c.st, last_round, whole_rounds);
}

// packed fp32 (k_mvn_packed.hip)
static int fwd_p(const FwdCall& c) {
    const PackLayout pk = pack_layout(c.cfg);
    ProfScope ps("k_mvn_enc_fwd_p", c.st);
    return launch_lds(k_mvn_enc_fwd_p, dim3((unsigned)((c.nb + EP_WAVES * EP_WP - 1) / (EP_WAVES * EP_WP))), dim3(EP_THREADS),
                      enc_p_lds_floats(c.dm.D, c.dm.J) * sizeof(float), c.st, c.dm, c.y, c.rows, c.gid0, c.W1, c.b1, c.packws,
                      c.packws + pk.bp, (uint32_t*)(c.packws + pk.gtab), c.eps_in, c.cfg->seed, c.cfg->step, c.cfg->step_dev,
                      c.cfg->stream, c.h, c.x, c.eps, c.ldT, c.ent, c.hT, c.epsT);
}

// unpacked, register-resident (k_mvn_enc_r.hip): H = 64, 16-byte loads
static bool fwd_r_ok(const FwdCall& c) {
    return !force_generic() && c.cfg->H == 64 && c.cfg->J % 4 == 0 && aligned16(c.y) && aligned16(c.W1) && aligned16(c.b1) &&
           aligned16(c.W21) && aligned16(c.W22) && aligned16(c.h) && enc_r_lds_floats(c.dm.D, c.dm.J) * sizeof(float) <= 160 * 1024;
}
static int fwd_r(const FwdCall& c) {
    return launch_lds(k_mvn_enc_fwd_r, dim3((unsigned)((c.nb + ER_WAVES * ER_WP - 1) / (ER_WAVES * ER_WP))), dim3(ER_THREADS),
                      enc_r_lds_floats(c.dm.D, c.dm.J) * sizeof(float), c.st, c.dm, c.y, c.rows, c.gid0, c.W1, c.b1, c.W21, c.b21,
                      c.W22, c.b22, c.eps_in, c.cfg->seed, c.cfg->step, c.cfg->step_dev, c.cfg->stream, c.h, c.x, c.eps, c.ldT, c.ent);
}

// shape-generic (k_mvn_enc.hip)
static int fwd_generic(const FwdCall& c) {
    return with_hidden_width(c.dm.Hp, [&](auto ht) -> int {
        return launch_lds(k_mvn_enc_fwd<decltype(ht)::value>, dim3((unsigned)((c.nb + ENC_P - 1) / ENC_P)), dim3(ENC_THREADS),
                          enc_fwd_lds_floats(c.dm.D, c.dm.Hp) * sizeof(float), c.st, c.dm, c.y, c.rows, c.gid0, c.W1, c.b1, c.W21,
                          c.b21, c.W22, c.b22, c.eps_in, c.cfg->seed, c.cfg->step, c.cfg->step_dev, c.cfg->stream, c.h, c.x, c.eps,
                          c.ldT, c.ent);
    });
}

// The kernels of the forward, chosen once.  The packed path on the f16x2 kernels (p.fwb) writes the likelihood's x image and
// the fp16 terms of hT itself; the entry point makes them behind the other paths.
static int mvn_enc_forward_kernels(const FwdCall& c) {
    if (c.packed && c.p.fwb) {
        const int rc = fwd_pack_fused(c);
        if (rc) return rc;
        return c.nb <= FB_SPLIT_MAX ? fwd_b_small(c) : fwd_b_large(c);
    }
    if (c.packed) {
        const int rc = fwd_pack_heads(c);
        return rc ? rc : fwd_p(c);
    }
    return fwd_r_ok(c) ? fwd_r(c) : fwd_generic(c);
}

int vx_mvn_enc_forward(const vx_irt_cfg* cfg, const uint8_t* y, const int64_t* rows, int64_t nb, int64_t gid0,
                       const float* W1, const float* b1, const float* W21, const float* b21, const float* W22,
                       const float* b22, const float* eps_in, float* h, float* x, float* eps, float* ldT,
                       float* ent, float* hT, float* epsT, float* packws, uint8_t* ximg, uint16_t* hs_out, void* hs) {
    if (!enc_cfg_ok(cfg) || !y || !W1 || !b1 || !W21 || !b21 || !W22 || !b22 || !h || !x || !eps || !ldT || !ent ||
        nb < 0)
        return VX_EINVAL;
    if (nb == 0) return VX_OK;
    if (ximg && !(lik_h_shape(cfg) && aligned16(ximg))) return VX_EINVAL;     // vx_irt_lik_ximg_bytes(cfg, nb) == 0: no image
    if (hs_out && (!hT || cfg->H != 64)) return VX_EINVAL;
    const MvnPlan p = mvn_plan(cfg, nb);
    // the packed path: the shape allows it and the buffers it reads 16 bytes at a time are aligned
    const bool packed = p.packed && packws && aligned16(packws) && aligned16(y) && aligned16(W1) && aligned16(b1) &&
                        aligned16(W21) && aligned16(W22) && aligned16(h);
    // the caller will hand hs to vx_mvn_enc_backward (gd_ready bit 1), which reads it and the powers of two in packws
    // unconditionally: they exist on the packed path only (checked BEFORE anything is launched)
    if (hs_out && !packed) return VX_EINVAL;
    const bool fused = packed && p.fwb;                            // the f16x2 kernels write the x image and hs themselves
    uint32_t* ovf = ximg ? (uint32_t*)(ximg + lik_ximg_ovf_bytes(nb)) : nullptr;   // k_irt_lik_h.hip
    if (ovf && hipMemsetAsync(ovf, 0, sizeof(uint32_t), (hipStream_t)hs) != hipSuccess) return VX_EINVAL;
    // the step's row indices from the pinned host ring (vx_irt_cfg.rows_ring): inside the first launch of the fused pack, or
    // as a launch of its own in front of every other forward path
    const int64_t* ring = nullptr;
    if (cfg->rows_ring) {
        if (!rows || !cfg->step_dev || cfg->rows_ring_slots < 1 || cfg->rows_ring_stride < nb) return VX_EINVAL;
        void* dp = nullptr;
        if (hipHostGetDevicePointer(&dp, const_cast<int64_t*>(cfg->rows_ring), 0) != hipSuccess || !dp) return VX_EINVAL;
        ring = (const int64_t*)dp;
        if (!fused) {
            hipLaunchKernelGGL(k_rows_from_ring, dim3(1), dim3(256), 0, (hipStream_t)hs, ring, (int64_t)cfg->rows_ring_stride,
                               (int)cfg->rows_ring_slots, cfg->step_dev, const_cast<int64_t*>(rows), nb);
            VX_CHECK_LAUNCH();
            ring = nullptr;
        }
    }
    const FwdCall c{cfg, p, make_enc_dims(cfg, nb), packed, y, rows, nb, gid0, W1, b1, W21, b21, W22, b22, eps_in, h, x, eps, ldT,
                    ent, hT, epsT, packws, ximg, hs_out, (hipStream_t)hs, ring};
    const int rc = mvn_enc_forward_kernels(c);
    if (rc) return rc;                                               // nothing is launched on buffers an error left unwritten
    if (ximg && !fused) {
        hipLaunchKernelGGL(k_lik_ximg_h, dim3((unsigned)((nb + LB_P - 1) / LB_P)), dim3(256), 0, (hipStream_t)hs, (int)cfg->D, nb,
                           (const float*)x, ximg, ovf);
        VX_CHECK_LAUNCH();
    }
    if (hs_out && !fused) {
        hipLaunchKernelGGL(k_split2_f16, dim3(num_cu() * 8), dim3(256), 0, (hipStream_t)hs, (const float*)hT, nb * 64,
                           (const float*)(packws + pack_layout(cfg).hscale), hs_out);
        VX_CHECK_LAUNCH();
    }
    return VX_OK;
}

// ------------------------------------------------------------------------------------------------
// person slices of the likelihood's specialised kernels: spread(), in whole XCD rounds (see their block decode)
static int xcd_spread(int64_t n_ptiles, int64_t groups) {
    const int n = spread(n_ptiles, groups);
    return n >= 8 ? n & ~7 : n;
}

// The plan of vx_irt_lik_grad for (cfg, nb) and the layout of its workspace (vx_irt_lik_workspace_floats), float offsets.
//   The register-resident (r) and the generic kernel: slabs [n_pr][slab_len] | with several item groups, gx partials
//   [groups][nb][D] | ll partials [groups][nb]; the generic kernel then a person-major gx (gx_tmp) when only gxT is asked for.
//   The bf16x3 / f16x2 kernels (b: a full batch whose item-major responses came): slabs [b_n_pr][slab_len] | x image of
//   n_ptiles 64-person tiles | gx partials [b_groups][LB_DP][nbp] | ll partials [b_groups][nbp] | overflow word.
// The workspace holds whichever of the two the call takes.
struct LikPlan {
    bool h;                      // the f16x2 kernel (k_irt_lik_h.hip) and its x image: 1PL / 2PL, D + 1 in (96, 112]
    bool b;                      // the bf16x3 path (k_irt_lik_b.hip): D + 1 in (96, 112]
    bool r;                      // the register-resident kernel (k_irt_lik_r.hip): D + 1 in (64, 128]
    int kt, nch;                 // the generic kernel's template arguments (k_irt_lik.hip)
    int groups, n_pr;            // item groups x person slices of the r or the generic kernel
    int64_t slab_len, gx_part, ll_part, gx_tmp;
    int b_groups = 0, b_n_pr = 0;
    int64_t n_ptiles, nbp;       // the b path's 64-person tiles
    int64_t b_ximg = -1, b_gx_part = -1, b_ll_part = -1, b_ovf = -1;
    int64_t total;
    int64_t ximg_bytes;          // the forward's f16x2 x image (h): tile images | overflow word (vx_irt_lik_ximg_bytes)
};
static LikPlan lik_plan(const vx_irt_cfg* cfg, int64_t nb) {
    static_assert(LB_XT_BYTES % 4 == 0, "the x image's tiles fill whole floats");
    LikPlan p;
    p.h = lik_h_shape(cfg);
    p.ximg_bytes = p.h ? lik_ximg_ovf_bytes(nb) + LH_FLAG_BYTES : 0;
    p.b = !force_generic() && cfg->D >= 96 && cfg->D <= 16 * LB_NKS - 1;
    p.r = !force_generic() && cfg->D >= 64 && cfg->D <= 127;
    p.slab_len = (int64_t)cfg->D * cfg->J + 3 * (int64_t)cfg->J;
    const int dk = cfg->D + 1;
    p.kt = dk <= 32 ? 1 : (dk <= 64 ? 2 : 4);
    p.nch = cfg->J <= LIK_JC ? 1 : 2;      // 4 chunks of register-resident GA tiles spill; 2 do not
    if (p.r) {                             // one 128-item chunk per workgroup
        p.groups = (cfg->J + LR_JC - 1) / LR_JC;
        p.n_pr = xcd_spread((nb + LR_P - 1) / LR_P, p.groups);
    } else {
        p.groups = (cfg->J + p.nch * LIK_JC - 1) / (p.nch * LIK_JC);
        p.n_pr = spread((nb + LIK_P - 1) / LIK_P, p.groups);
    }
    p.gx_part = (int64_t)p.n_pr * p.slab_len;
    p.ll_part = p.gx_part + (int64_t)p.groups * nb * cfg->D;
    const int64_t used = p.gx_part + (p.groups > 1 ? (int64_t)p.groups * nb * (cfg->D + 1) : 0);
    p.gx_tmp = p.r ? -1 : ((used + 3) & ~(int64_t)3);
    p.total = p.r ? used : used + nb * cfg->D + 4;
    p.n_ptiles = (nb + LB_P - 1) / LB_P;
    p.nbp = p.n_ptiles * LB_P;
    if (p.b) {
        p.b_groups = (cfg->J + LB_JC - 1) / LB_JC;
        p.b_n_pr = xcd_spread(p.n_ptiles, p.b_groups);
        p.b_ximg = ((int64_t)p.b_n_pr * p.slab_len + 3) & ~(int64_t)3;
        p.b_gx_part = p.b_ximg + p.n_ptiles * (LB_XT_BYTES / 4);
        p.b_ll_part = p.b_gx_part + (int64_t)p.b_groups * LB_DP * p.nbp;
        p.b_ovf = p.b_ll_part + (int64_t)p.b_groups * p.nbp;                   // of an x image made here
        if (p.b_ovf + 16 > p.total) p.total = p.b_ovf + 16;
    }
    return p;
}

static bool lik_cfg_ok(const vx_irt_cfg* cfg) {
    return cfg && cfg->D >= 2 && cfg->D <= 127 && cfg->J >= 1 && cfg->model >= VX_IRT_2PL &&
           cfg->model <= VX_IRT_4PL;
}

int64_t vx_irt_lik_ximg_bytes(const vx_irt_cfg* cfg, int64_t nb) {
    if (!lik_cfg_ok(cfg) || nb < 0) return VX_EINVAL;
    return lik_plan(cfg, nb).ximg_bytes;
}

int64_t vx_irt_lik_workspace_floats(const vx_irt_cfg* cfg, int64_t nb) {
    if (!lik_cfg_ok(cfg) || nb < 0) return VX_EINVAL;
    return lik_plan(cfg, nb).total;
}

// One call of vx_irt_lik_grad (arguments validated by the entry point below) and its plan
struct LikCall {
    const vx_irt_cfg* cfg; LikPlan p;
    const uint8_t* y; const int64_t* rows; int64_t nb;
    const float *x, *a, *b, *c_un, *d_un;
    float *gx, *gxT, *ll, *gitem, *workspace;
    const uint8_t* yT; int64_t yT_stride; const uint8_t* ximg_in;
    const float *epsT, *ldT; float* gdT; uint32_t* opmax; hipStream_t st;
};
// what a path returns: the call's status, and whether the path wrote gdT (and the operand maxima) itself
struct LikDone { int rc; bool gd_done; LikDone(int r, bool gd = false) : rc(r), gd_done(gd) {} };

// the bf16x3 / f16x2 kernels (k_irt_lik_b.hip, k_irt_lik_h.hip): a full batch whose item-major responses came
static bool lik_b_ok(const LikCall& c) {
    return c.p.b && !c.rows && c.yT && c.gxT && c.yT_stride % 64 == 0 && c.yT_stride >= c.p.nbp && aligned16(c.yT) && c.nb > 0 &&
           aligned16(c.workspace) && aligned16(c.gxT);
}
static LikDone lik_grad_b(const LikCall& c) {
    const vx_irt_cfg* cfg = c.cfg; const LikPlan& p = c.p;
    const int64_t nb = c.nb, n_ptiles = p.n_ptiles, nbp = p.nbp;
    const int groups = p.b_groups, n_pr = p.b_n_pr;
    LikBDims dm;
    dm.D = cfg->D; dm.J = cfg->J; dm.model = cfg->model; dm.groups = groups; dm.n_pr = n_pr; dm.gxt = 1;
    dm.Dc = cfg->Dc; dm.scale = cfg->scale; dm.nb = nb;
    dm.slab_len = p.slab_len;
    float* slabs = c.workspace;
    uint8_t* ximg_ws = (uint8_t*)(c.workspace + p.b_ximg);
    float* gx_part = c.workspace + p.b_gx_part;
    // 1PL / 2PL link: the f16x2 kernel and its image (the forward's, or made here); its gx stores address 16 nbp bytes
    // with 32 bits.  3PL / 4PL: the bf16x3 kernel on its own three-term image (the forward writes none for them).
    const bool f16 = p.h && nbp < ((int64_t)1 << 27);
    const uint8_t* ximg = (f16 && c.ximg_in && aligned16(c.ximg_in)) ? c.ximg_in : ximg_ws;
    float* ll_part = c.workspace + p.b_ll_part;
    // the overflow word of the f16 image: behind the forward's image, or -- an image made here -- at the end of the workspace
    uint32_t* ovf = (ximg == ximg_ws) ? (uint32_t*)(c.workspace + p.b_ovf)
                                      : (uint32_t*)(const_cast<uint8_t*>(c.ximg_in) + lik_ximg_ovf_bytes(nb));
    hipStream_t st = c.st;
    hipError_t he = hipMemsetAsync(slabs, 0, sizeof(float) * (size_t)n_pr * dm.slab_len, st);
    if (he != hipSuccess) return (int)he;
    if (ximg == ximg_ws) {
        if (f16) {
            if (hipMemsetAsync(ovf, 0, sizeof(uint32_t), st) != hipSuccess) return VX_EINVAL;
            hipLaunchKernelGGL(k_lik_ximg_h, dim3((unsigned)n_ptiles), dim3(256), 0, st, (int)cfg->D, nb, c.x, ximg_ws, ovf);
        } else {
            hipLaunchKernelGGL(k_lik_ximg, dim3((unsigned)n_ptiles), dim3(256), 0, st, (int)cfg->D, nb, c.x, ximg_ws, (const uint32_t*)nullptr);
        }
        VX_CHECK_LAUNCH();
    }
    int rc;
    const dim3 grid((unsigned)(groups * n_pr));
    if (f16) {
        rc = set_lds(k_irt_lik_h<0>, LH_LDS_BYTES);
        if (rc) return rc;
        ProfScope ps("k_irt_lik_h", st);
        hipLaunchKernelGGL((k_irt_lik_h<0>), grid, dim3(LH_THREADS), LH_LDS_BYTES, st, dm, c.yT, c.yT_stride, ximg, c.a, c.b,
                           gx_part, ll_part, slabs, (const uint32_t*)ovf);
        VX_CHECK_LAUNCH();
        // the stand-by for a latent outside the f16 image's range (|x| >= 511.75): the bf16x3 kernel on its own image, both
        // returning at once unless the overflow word is set -- two empty launches a step otherwise.  Its image takes the
        // workspace's image region (an f16 image made here is dead by then; the overflow word is not in that region).
        rc = set_lds(k_irt_lik_b<0>, LB_LDS_BYTES);
        if (rc) return rc;
        hipLaunchKernelGGL(k_lik_ximg, dim3((unsigned)(n_ptiles < 4 * num_cu() ? n_ptiles : 4 * num_cu())), dim3(256), 0, st, (int)cfg->D,
                           nb, c.x, ximg_ws, (const uint32_t*)ovf);
        hipLaunchKernelGGL((k_irt_lik_b<0>), grid, dim3(LB_THREADS), LB_LDS_BYTES, st, dm, c.yT, c.yT_stride, (const uint8_t*)ximg_ws,
                           c.a, c.b, c.c_un, c.d_un, gx_part, ll_part, slabs, (long long*)nullptr, (const uint32_t*)ovf);
    } else {
        const auto kernel = cfg->model >= VX_IRT_3PL ? k_irt_lik_b<1> : k_irt_lik_b<0>;
        rc = set_lds(kernel, LB_LDS_BYTES);
        if (rc) return rc;
        ProfScope ps("k_irt_lik_b", st);
        hipLaunchKernelGGL(kernel, grid, dim3(LB_THREADS), LB_LDS_BYTES, st, dm, c.yT, c.yT_stride, ximg, c.a, c.b, c.c_un, c.d_un,
                           gx_part, ll_part, slabs, (long long*)nullptr, (const uint32_t*)nullptr);
    }
    VX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_lik_reduce_parts, dim3((unsigned)n_ptiles), dim3(256), (size_t)64 * (cfg->D | 1) * sizeof(float), st, (const float*)gx_part, (const float*)ll_part,
                       c.x, groups, (int)cfg->D, nb, nbp, cfg->scale, c.gxT, c.ll, c.epsT, c.ldT, c.gdT, c.opmax);
    VX_CHECK_LAUNCH();
    if (c.gx) {                                        // both orders requested: gx[nb][D] = transpose(gxT[D][nb])
        hipLaunchKernelGGL(k_transpose, dim3(num_cu() * 8), dim3(256), 0, st, c.gxT, c.gx, (int64_t)cfg->D, nb);
        VX_CHECK_LAUNCH();
    }
    return LikDone(vx_reduce_slabs(slabs, n_pr, dm.slab_len, -1.0f, c.gitem, (void*)st), true);
}

// the register-resident kernel (k_irt_lik_r.hip)
static LikDone lik_grad_r(const LikCall& c) {
    const vx_irt_cfg* cfg = c.cfg; const LikPlan& p = c.p;
    const int64_t nb = c.nb;
    const int groups = p.groups, n_pr = p.n_pr;
    const uint8_t* y = c.y; const int64_t* rows = c.rows; const float *x = c.x, *a = c.a, *b = c.b, *c_un = c.c_un, *d_un = c.d_un;
    float *gx = c.gx, *gxT = c.gxT;
    LikRDims dm;
    dm.D = cfg->D; dm.J = cfg->J; dm.K8 = (cfg->D + 8) & ~7; dm.model = cfg->model;
    { const int nq = dm.K8 >> 3; dm.XS = 8 * (nq <= 13 ? 13 : 16) + 4; }
    dm.groups = groups; dm.n_pr = n_pr; dm.Dc = cfg->Dc; dm.scale = cfg->scale; dm.nb = nb;
    dm.slab_len = p.slab_len;
    dm.fast = (cfg->D % 4 == 0 && cfg->J % 4 == 0 && cfg->J >= 8 && aligned16(x) && aligned16(y) &&
               aligned16(gx) && aligned16(c.workspace)) ? 1 : 0;
    dm.gxt = gxT ? 1 : 0;                              // partials (and their sum) dimension-major
    float* slabs = c.workspace;
    float* gx_sum = gxT ? gxT : gx;
    float* gx_part = groups > 1 ? c.workspace + p.gx_part : gx_sum;
    float* ll_part = groups > 1 ? c.workspace + p.ll_part : c.ll;
    hipStream_t st = c.st;
    // several item chunks and dimension-major partials: ONE finishing launch sums the partials, makes the DIAG-row operand
    // and reduces the item slabs (k_lik_finish); otherwise the slabs are cleared and reduced as before
    const bool finish1 = nb > 0 && groups > 1 && !(gxT && gx);
    if (!finish1) {
        hipError_t he = hipMemsetAsync(slabs, 0, sizeof(float) * (size_t)n_pr * dm.slab_len, st);
        if (he != hipSuccess) return (int)he;
    }
    if (nb > 0) {
        const size_t lds = likr_lds_bytes(dm.XS);
        const dim3 grid((unsigned)(groups * n_pr));
        int rc = VX_EINVAL;
        const int nq = dm.K8 >> 3;                     // 9..16; instantiated: 13, 16 (extra rows are zeros)
#define LAUNCH_LIKR(GEN, NQ, FAST)                                                                              \
    rc = set_lds(k_irt_lik_r<GEN, NQ, FAST>, lds);                                                              \
    if (rc) return rc;                                                                                          \
    ProfScope ps("k_irt_lik_r", st);                                                                            \
    hipLaunchKernelGGL((k_irt_lik_r<GEN, NQ, FAST>), grid, dim3(LR_THREADS), lds, st, dm, y, rows, x, a, b,     \
                       c_un, d_un, gx_part, ll_part, slabs)
#define DISPATCH_LIKR(GEN, FAST)                            \
    if (nq <= 13) { LAUNCH_LIKR(GEN, 13, FAST); }           \
    else { LAUNCH_LIKR(GEN, 16, FAST); }
        const int fastv = dm.fast ? (rows ? 2 : 1) : 0;
        if (cfg->model >= VX_IRT_3PL) {
            if (fastv == 2) { DISPATCH_LIKR(1, 2) } else if (fastv == 1) { DISPATCH_LIKR(1, 1) } else { DISPATCH_LIKR(1, 0) }
        } else {
            if (fastv == 2) { DISPATCH_LIKR(0, 2) } else if (fastv == 1) { DISPATCH_LIKR(0, 1) } else { DISPATCH_LIKR(0, 0) }
        }
#undef DISPATCH_LIKR
#undef LAUNCH_LIKR
        VX_CHECK_LAUNCH();
        if (finish1) {
            const int64_t n_gx = nb * cfg->D;
            const bool with_gd = c.gdT && gxT && !c.opmax;   // (the maxima, when asked for, come from k_absmax3 behind k_mvn_gd)
            const int nblk_gx = grid_1d(n_gx, 256), nblk_ll = grid_1d(nb, 256), nblk_s = grid_1d(dm.slab_len, 64);
            // (the kernel writes the a and b columns of every item, and the c / d columns only for the 3PL / 4PL links)
            const int64_t len_w = cfg->model >= VX_IRT_3PL ? dm.slab_len : (int64_t)(cfg->D + 1) * cfg->J;
            hipLaunchKernelGGL(k_lik_finish, dim3((unsigned)(nblk_gx + nblk_ll + nblk_s)), dim3(256), 0, st, (const float*)gx_part,
                               groups, n_gx, gx_sum, with_gd ? c.epsT : (const float*)nullptr, c.ldT, with_gd ? c.gdT : (float*)nullptr,
                               cfg->scale, (const float*)ll_part, nb, c.ll, (const float*)slabs, (int64_t)n_pr, dm.slab_len, len_w,
                               c.gitem, nblk_gx, nblk_ll);
            VX_CHECK_LAUNCH();
            return LikDone(VX_OK, with_gd);
        }
        if (groups > 1) {
            int r2 = vx_reduce_slabs(gx_part, groups, nb * cfg->D, 1.0f, gx_sum, (void*)st);
            if (r2) return r2;
            r2 = vx_reduce_slabs(ll_part, groups, nb, 1.0f, c.ll, (void*)st);
            if (r2) return r2;
        }
        if (gxT && gx) {                               // both orders requested: gx[nb][D] = transpose(gxT[D][nb])
            hipLaunchKernelGGL(k_transpose, dim3(num_cu() * 8), dim3(256), 0, st, gxT, gx, (int64_t)cfg->D, nb);
            VX_CHECK_LAUNCH();
        }
    }
    return vx_reduce_slabs(slabs, n_pr, dm.slab_len, -1.0f, c.gitem, (void*)st);
}

// the shape-generic kernel (k_irt_lik.hip)
static LikDone lik_grad_generic(const LikCall& c) {
    const vx_irt_cfg* cfg = c.cfg; const LikPlan& p = c.p;
    const int64_t nb = c.nb;
    const int groups = p.groups, n_pr = p.n_pr, kt = p.kt, nch = p.nch;
    const uint8_t* y = c.y; const int64_t* rows = c.rows; const float *x = c.x, *a = c.a, *b = c.b, *c_un = c.c_un, *d_un = c.d_un;
    float* gx = c.gx ? c.gx : c.workspace + p.gx_tmp;  // person-major result of the kernels below
    LikDims dm;
    dm.D = cfg->D; dm.J = cfg->J; dm.DS = lik_ds(cfg->D); dm.Dk2 = (cfg->D + 2) & ~1; dm.model = cfg->model;
    dm.Dc = cfg->Dc; dm.scale = cfg->scale; dm.nb = nb;
    dm.slab_len = p.slab_len;
    dm.fast = (!force_generic() && cfg->D % 4 == 0 && cfg->J % 4 == 0 && aligned16(x) && aligned16(a) && aligned16(b) &&
               aligned16(y) && aligned16(gx) && (nb * cfg->D) % 4 == 0) ? 1 : 0;
    const int gen = cfg->model >= VX_IRT_3PL ? 1 : 0;
    float* slabs = c.workspace;
    float* gx_part = groups > 1 ? c.workspace + p.gx_part : gx;
    float* ll_part = groups > 1 ? c.workspace + p.ll_part : c.ll;
    hipStream_t st = c.st;
    // slabs are only partially written when a model has no c/d segment: clear them first
    hipError_t he = hipMemsetAsync(slabs, 0, sizeof(float) * (size_t)n_pr * dm.slab_len, st);
    if (he != hipSuccess) return (int)he;
    if (nb > 0) {
        const size_t lds = lik_lds_floats(cfg->D, nch, gen) * sizeof(float);
        const dim3 grid((unsigned)groups, (unsigned)n_pr);
        int rc = VX_EINVAL;
#define LAUNCH_LIK(KT, NCH, GEN)                                                                             \
    rc = set_lds(k_irt_lik<KT, NCH, GEN>, lds);                                                              \
    if (rc) return rc;                                                                                       \
    hipLaunchKernelGGL((k_irt_lik<KT, NCH, GEN>), grid, dim3(LIK_THREADS), lds, st, dm, y, rows, x, a, b, c_un, \
                       d_un, gx_part, ll_part, slabs)
#define DISPATCH_NCH(KT, GEN)                                     \
    if (nch == 1) { LAUNCH_LIK(KT, 1, GEN); }                     \
    else { LAUNCH_LIK(KT, 2, GEN); }
#define DISPATCH_KT(GEN)                                          \
    if (kt == 1) { DISPATCH_NCH(1, GEN) }                         \
    else if (kt == 2) { DISPATCH_NCH(2, GEN) }                    \
    else { DISPATCH_NCH(4, GEN) }
        if (gen) { DISPATCH_KT(1) } else { DISPATCH_KT(0) }
#undef DISPATCH_KT
#undef DISPATCH_NCH
#undef LAUNCH_LIK
        VX_CHECK_LAUNCH();
        if (groups > 1) {
            int r2 = vx_reduce_slabs(gx_part, groups, nb * cfg->D, 1.0f, gx, (void*)st);
            if (r2) return r2;
            r2 = vx_reduce_slabs(ll_part, groups, nb, 1.0f, c.ll, (void*)st);
            if (r2) return r2;
        }
    }
    if (c.gxT && nb > 0) {
        hipLaunchKernelGGL(k_transpose, dim3(num_cu() * 8), dim3(256), 0, st, gx, c.gxT, nb, (int64_t)cfg->D);
        VX_CHECK_LAUNCH();
    }
    // loss gradients = -(d ELBO / d .)
    return vx_reduce_slabs(slabs, n_pr, dm.slab_len, -1.0f, c.gitem, (void*)st);
}

int vx_irt_lik_grad(const vx_irt_cfg* cfg, const uint8_t* y, const int64_t* rows, int64_t nb, const float* x,
                    const float* a, const float* b, const float* c_un, const float* d_un, float* gx, float* gxT,
                    float* ll, float* gitem, float* workspace, const uint8_t* yT, int64_t yT_stride, const uint8_t* ximg_in,
                    const float* epsT, const float* ldT, float* gdT, uint32_t* opmax, void* hs) {
    if (!lik_cfg_ok(cfg) || !y || !x || !a || !b || (!gx && !gxT) || !ll || !gitem || !workspace || nb < 0)
        return VX_EINVAL;
    if (opmax && !gdT) return VX_EINVAL;
    if (gdT && (!gxT || !epsT || !ldT || (nb * (int64_t)cfg->D) % 4 != 0 || !aligned16(gdT) || !aligned16(gxT) ||
                !aligned16(epsT) || !aligned16(ldT)))
        return VX_EINVAL;
    if (cfg->model >= VX_IRT_3PL && !c_un) return VX_EINVAL;
    if (cfg->model == VX_IRT_4PL && !d_un) return VX_EINVAL;
    const LikCall c{cfg, lik_plan(cfg, nb), y, rows, nb, x, a, b, c_un, d_un, gx, gxT, ll, gitem, workspace, yT, yT_stride, ximg_in,
                    epsT, ldT, gdT, opmax, (hipStream_t)hs};
    const LikDone done = lik_b_ok(c) ? lik_grad_b(c) : (c.p.r ? lik_grad_r(c) : lik_grad_generic(c));
    if (done.rc) return done.rc;
    const bool gd_done = done.gd_done;
    // the fused DIAG-row operand of the guide backward, for the paths that do not make it themselves
    if (gdT && !gd_done && nb > 0) {
        hipLaunchKernelGGL(k_mvn_gd, dim3(num_cu() * 8), dim3(256), 0, (hipStream_t)hs, (const float4*)gxT, (const float4*)epsT,
                           (const float4*)ldT, cfg->scale, nb * cfg->D / 4, (float4*)gdT);
        VX_CHECK_LAUNCH();
    }
    if (opmax && !gd_done && nb > 0) {                     // (the fused pass collects the maxima itself)
        hipLaunchKernelGGL(k_absmax3, dim3(grid_1d(nb * cfg->D, 1024)), dim3(256), 0, (hipStream_t)hs, (const float*)gxT, (const float*)gdT, epsT,
                           nb * cfg->D, opmax);
        VX_CHECK_LAUNCH();
    }
    return VX_OK;
}

// ------------------------------------------------------------------------------------------------
int vx_mvn_enc_bwd_layout(const vx_irt_cfg* cfg, int64_t nb) {
    if (!enc_cfg_ok(cfg) || nb < 0) return VX_EINVAL;
    return mvn_plan(cfg, nb).bwh_t ? 1 : 0;
}

// float offset, inside the workspace of vx_mvn_enc_backward, of gdT[D][nb] (the DIAG-row operand of the dimension-major
// kernels); -1 when this (cfg, nb) does not run on them
int64_t vx_mvn_enc_bwd_gd_offset(const vx_irt_cfg* cfg, int64_t nb) {
    if (!enc_cfg_ok(cfg) || nb < 0) return VX_EINVAL;
    const int64_t o = mvn_plan(cfg, nb).gd;
    return (o >= 0 && o % 4 == 0 && (nb * cfg->D) % 4 == 0) ? o : -1;
}

int64_t vx_mvn_enc_bwd_hs_offset(const vx_irt_cfg* cfg, int64_t nb) {
    if (!enc_cfg_ok(cfg) || nb < 0) return VX_EINVAL;
    return mvn_plan(cfg, nb).hs;
}

int64_t vx_mvn_pack_floats(const vx_irt_cfg* cfg) {
    if (!enc_cfg_ok(cfg)) return VX_EINVAL;
    return pack_layout(cfg).total;
}

int64_t vx_mvn_pack_opmax_offset(const vx_irt_cfg* cfg, int64_t nb) {
    if (!enc_cfg_ok(cfg) || nb < 0) return VX_EINVAL;
    const MvnPlan p = mvn_plan(cfg, nb);
    return (p.hb_fw && p.bwb) ? pack_layout(cfg).maxw : -1;
}

int64_t vx_mvn_enc_param_floats(const vx_irt_cfg* cfg) {
    if (!enc_cfg_ok(cfg)) return VX_EINVAL;
    const int64_t D = cfg->D, J = cfg->J, H = cfg->H, T = tril_len(cfg->D);
    return H * J + H + D * H + D + T * H + T;
}

int64_t vx_mvn_enc_bwd_workspace_floats(const vx_irt_cfg* cfg, int64_t nb) {
    if (!enc_cfg_ok(cfg) || nb < 0) return VX_EINVAL;
    return mvn_plan(cfg, nb).total;
}

// the loss of the step, summed by the call's last launch (vx_mvn_enc_backward_loss)
struct LossTail { const float* ll; const float* ent; float alpha; float* loss; float* sum_ws; };

// The arguments of one vx_mvn_enc_backward(_loss) call
struct BwdArgs {
    const uint8_t* y; const int64_t* rows; int64_t nb;
    const float *W21, *W22, *h, *eps, *ldT, *gx, *hT, *epsT, *gxT;
    const uint8_t* yT; int64_t yT_stride;
    float *genc, *workspace; const float* packws; int32_t gd_ready; const LossTail* tail;
};

// The route of one backward call: every choice that (plan, pointer presence and alignment, nb, rows, yT_stride, gd_ready
// bits) decide, resolved by bwd_route() before the first launch.  What a fork's success decides at run time is not in here.
enum class BwdLayout { Empty, DimMajor, PackedPersonMajor, Fast, Generic };    // Empty: nb == 0; DimMajor: hT / epsT / gxT / gdT
enum class HidKernel { None, B_small, B2, B_large, T, P, Fast, Generic };      // h_b<true> | h_b2 (+ h_b<false>) | h_b<false> | h_t | h_p | ..
enum class WgtKernel { None, B, T, T_fc1, FastPacked, Fast, Generic };         // w_b | w_t | k_bwd_wt_fc1 | w_fast<true> | w_fast<false> | w<HT>
enum class Fc1Kernel { None, C, T, Rode, Small, Wide };                        // fc1_bwd_c | fc1_bwd_t | in k_bwd_wt_fc1 | fc1_bwd<2, 1> | fc1_bwd<HT>
struct BwdRoute {
    bool refused;                // VX_EINVAL: the plan assumed the packed row space, or the person-major kernel has no gx
    BwdLayout layout;
    bool packed;                 // DimMajor or PackedPersonMajor: the packed head layout, the one-launch tail (k_enc_bwd_tail)
    HidKernel hid;
    int64_t hid_n_done;          // B2: the persons of its whole chip rounds; the rest is a last round of h_b<false> ...
    bool hid_last_side;          // ... which wants the side stream (0)
    bool pack_hb, pack_heads;    // k_pack_heads_hb / k_pack_heads in front of the hidden gradient
    bool f1t;                    // the hidden gradient leaves ghpreT (dimension-major) for the fc1 gradient
    WgtKernel wgt;
    int n_rowslabs, n_prw;       // its grid
    bool gd_first;               // k_mvn_gd in front of everything (gd_ready bit 0 not set)
    bool split_hs, absmax;       // B: k_split2_f16 (bit 1 not set) / k_clear_words + k_absmax3 (maxima not collected) in front of it
    bool pair;                   // B wants stream 1, beside the hidden gradient (all three gd_ready bits, images from the forward)
    Fc1Kernel fc1;
    bool fc1_side;               // C wants stream 0, beside the head weight gradient
    bool maxw_in_pack;           // the operand maxima and the unit images live in packws (the forward packed for this backward) ...
    bool maxw_ready;             // ... and the maxima are collected when the weight and fc1 gradients start (an h_b kernel ran)
};
static BwdRoute bwd_route(const vx_irt_cfg* cfg, const MvnPlan& p, const BwdArgs& a) {
    const int64_t nb = a.nb;
    const bool f1_small = fc1_small_batch((cfg->H + 31) / 32 * 32, p.n_jg, p.n_prf);
    BwdRoute r = {};
    r.packed = p.packed && a.packws && aligned16(a.packws) && aligned16(a.h) && aligned16(a.eps) && aligned16(a.gx) &&
               aligned16(a.workspace) && nb > 0;
    const bool use_t = r.packed && a.hT && a.epsT && a.gxT && p.bwt && aligned16(a.hT) && aligned16(a.epsT) && aligned16(a.gxT) &&
                       aligned16(a.ldT);
    const bool fast = !r.packed && p.encb_fast && aligned16(a.W21) && aligned16(a.W22) && aligned16(a.h) && aligned16(a.eps) &&
                      aligned16(a.gx) && aligned16(a.workspace);
    r.layout = nb == 0 ? BwdLayout::Empty : use_t ? BwdLayout::DimMajor : r.packed ? BwdLayout::PackedPersonMajor
               : fast ? BwdLayout::Fast : BwdLayout::Generic;
    r.maxw_in_pack = a.packws && p.hb_fw;
    r.n_rowslabs = use_t ? p.n_rowslabs_t : p.n_rowslabs;
    r.n_prw = use_t ? p.n_prw_t : p.n_prw;
    r.gd_first = use_t && !(a.gd_ready & 1);
    // the hidden gradient
    if (use_t && p.bwh_t) {
        r.f1t = a.yT && !a.rows && a.yT_stride % 16 == 0 && a.yT_stride >= nb && aligned16(a.yT) && cfg->J >= 32 &&
                f1_lds_bytes(cfg->J) <= 160 * 1024;
        r.hid = HidKernel::T;
        if (p.bwhb) {
            r.pack_hb = !r.maxw_in_pack;
            r.maxw_ready = true;
            // small batch: the eight waves of a workgroup share the units; large batch: 64 persons per wave, batches of four
            // units per barrier (k_mvn_bwd_hb2.hip)
            r.hid = nb <= HB_SPLIT_MAX ? HidKernel::B_small
                    : (cfg->D <= 112 && hb2_lds_bytes(cfg->D) <= 160 * 1024) ? HidKernel::B2 : HidKernel::B_large;
            // B2's workgroups take 256 persons: a last round that fills less than half the chip goes to the 32-persons-
            // per-wave kernel instead (1M persons: 15 full rounds + 16 960 persons), as in the forward
            const int64_t round2 = (int64_t)256 * num_cu(), rem = nb % round2;
            r.hid_n_done = (rem > 0 && 2 * rem <= round2 && nb > round2) ? nb - rem : nb;
            r.hid_last_side = r.hid == HidKernel::B2 && r.hid_n_done < nb && p.side_streams;
        }
    } else if (r.packed) {
        r.hid = HidKernel::P;
        // the forward call packed for the f16x2 hidden gradient and made no packed copy of the heads (k_pack_fused.hip,
        // direct): this kernel reads one
        r.pack_heads = r.maxw_in_pack;
    } else if (nb > 0) {
        r.hid = fast ? HidKernel::Fast : HidKernel::Generic;
    }
    r.refused = (p.packed && !r.packed && nb > 0) || (r.hid == HidKernel::P && !a.gx);
    // the head weight gradient.  T_fc1: a small batch, the fc1 weight gradient (k_fc1_bwd<2, 1>) rides in the same launch
    const bool rides = !r.f1t && f1_small && BT_THREADS == ENC_THREADS;
    if (use_t) r.wgt = p.bwb ? WgtKernel::B : rides ? WgtKernel::T_fc1 : WgtKernel::T;
    else if (nb > 0) r.wgt = r.packed ? WgtKernel::FastPacked : fast ? WgtKernel::Fast : WgtKernel::Generic;
    r.split_hs = r.wgt == WgtKernel::B && !(a.gd_ready & 2);
    r.absmax = r.wgt == WgtKernel::B && !r.maxw_ready;
    r.pair = r.wgt == WgtKernel::B && (a.gd_ready & 7) == 7 && r.maxw_in_pack && p.bwh_t && p.side_streams;
    // (the plan sized its row slabs for the fast kernel where the shape allows that one)
    if (r.wgt == WgtKernel::Generic) r.n_rowslabs = (int)(((int64_t)tril_len(cfg->D) + cfg->D + BW_ROWS - 1) / BW_ROWS);
    // the fc1 gradient
    if (r.f1t) r.fc1 = p.fc1_16 ? Fc1Kernel::C : Fc1Kernel::T;
    else if (nb > 0) r.fc1 = r.wgt == WgtKernel::T_fc1 ? Fc1Kernel::Rode : f1_small ? Fc1Kernel::Small : Fc1Kernel::Wide;
    r.fc1_side = r.fc1 == Fc1Kernel::C && p.side_streams;
    return r;
}

// What the stages of one backward call read: the call, its plans and route, the regions of its buffers
extern "C++" struct BwdCtx {                                // (C++ linkage: it has a member template)
    const vx_irt_cfg* cfg; BwdArgs a; MvnPlan p; PackLayout pk; BwdRoute rt; EncDims dm; hipStream_t st;
    float *ghpre, *slabs_w, *slabs_f;
    float* gdT;                  // the DIAG-row operand of the dimension-major kernels
    uint16_t* hs3;               // two fp16 terms of hT 2^sh
    const float* sc;             // written by the forward call of this step (k_enc_scales): the powers of two of the f16x2 weight images
    uint32_t* maxw;              // the step's largest |gx|, |gd|, |eps|, |ghpre| (float bits): words 11 .. 14 of the scale block when the
                                 // forward call packed for this backward (cleared there), the last words of the workspace otherwise
    uint8_t* himg;               // the unit images: made by the forward call's pack launches (k_pack_fused.hip), or here
    const uint32_t* gtab;
    // one launch of an f16x2 hidden-gradient kernel (k_mvn_bwd_hb*.hip); more: the first person of a launch that is not the whole batch
    template <typename K, typename... More>
    int launch_hid_b(K kernel, int64_t n, int per_wg, unsigned threads, size_t lds, hipStream_t s, More... more) const {
        return launch_lds(kernel, dim3((unsigned)((n + per_wg - 1) / per_wg)), dim3(threads), lds, s, dm, (const uint8_t*)himg, sc, a.h,
                          a.eps, a.gxT, (const float*)gdT, rt.f1t ? (float*)nullptr : ghpre, a.hT, rt.f1t ? ghpre : (float*)nullptr,
                          maxw, more...);
    }
};
static BwdCtx bwd_ctx(const vx_irt_cfg* cfg, const BwdArgs& a, const MvnPlan& p, const BwdRoute& rt, hipStream_t st) {
    BwdCtx c{cfg, a, p, pack_layout(cfg), rt, make_enc_dims(cfg, a.nb), st};
    float* pw = const_cast<float*>(a.packws);
    c.ghpre = a.workspace; c.slabs_w = a.workspace + p.slabs_w; c.slabs_f = a.workspace + p.slabs_f;
    c.gdT = p.bwt ? a.workspace + p.gd : nullptr; c.hs3 = p.bwb ? (uint16_t*)(a.workspace + p.hs) : nullptr;
    c.sc = pw ? pw + c.pk.sc : nullptr;
    c.maxw = (uint32_t*)(rt.maxw_in_pack ? pw + c.pk.maxw : a.workspace + p.maxw);
    c.himg = !p.bwhb ? nullptr : (uint8_t*)(rt.maxw_in_pack ? pw + c.pk.himg : a.workspace + p.himg);
    c.gtab = pw ? (const uint32_t*)(pw + c.pk.gtab) : nullptr;
    return c;
}

// Stage 1, the hidden gradient: ghpre (or ghpreT: rt.f1t) from the heads' gradients.  beside_w: the head weight gradient
// already runs on its stream.
static int bwd_hidden(const BwdCtx& c, bool beside_w) {
    const BwdArgs& a = c.a; const BwdRoute& rt = c.rt; const EncDims& dm = c.dm;
    const int64_t nb = a.nb;
    hipStream_t st = c.st;
    const dim3 grid_p((unsigned)((nb + ENC_P - 1) / ENC_P));
    if (rt.pack_hb) {
        hipLaunchKernelGGL(k_pack_heads_hb, dim3(hb_units(dm.D)), dim3(256), 0, st, dm.D, a.W21, a.W22, c.sc, c.himg, c.maxw);
        VX_CHECK_LAUNCH();
    }
    if (rt.pack_heads) {
        hipLaunchKernelGGL(k_pack_heads, dim3((unsigned)c.pk.Rp), dim3(64), 0, st, (int)dm.D, 64, a.W21, (const float*)nullptr, a.W22,
                           (const float*)nullptr, const_cast<float*>(a.packws), (float*)nullptr, const_cast<uint32_t*>(c.gtab),
                           (float*)nullptr);
        VX_CHECK_LAUNCH();
    }
    switch (rt.hid) {
    case HidKernel::B_small: case HidKernel::B2: case HidKernel::B_large: {
        const size_t ldsh = hb_lds_bytes(dm.D);
        // (beside the head weight gradient the bracket spans both kernels: filed under a name of its own, not priced)
        ProfScope ps(beside_w ? "k_mvn_enc_bwd_h_b2 beside k_mvn_enc_bwd_w_b" : "k_mvn_enc_bwd_h_b", st);
        if (rt.hid == HidKernel::B_small) return c.launch_hid_b(k_mvn_enc_bwd_h_b<true>, nb, 32, HB_THREADS, ldsh, st, (int64_t)0);
        if (rt.hid == HidKernel::B_large) return c.launch_hid_b(k_mvn_enc_bwd_h_b<false>, nb, 32 * HB_WAVES, HB_THREADS, ldsh, st, (int64_t)0);
        constexpr int HNSET = 1;                              // eight waves of 32 persons (k_mvn_bwd_hb2.hip)
        const int64_t n_done = rt.hid_n_done;
        auto whole_rounds = [&]() -> int {
            return c.launch_hid_b(k_mvn_enc_bwd_h_b2<7, HNSET>, n_done, 256, 64 * HB2_WAVES_OF(HNSET), hb2_lds_bytes(dm.D), st);
        };
        if (n_done == nb) return whole_rounds();
        // the short last round on the second stream beside the whole rounds (launched first), as in the forward
        return with_last_round(rt.hid_last_side ? &side_stream(0, st) : nullptr, st, [&](hipStream_t ts) -> int {
            return c.launch_hid_b(k_mvn_enc_bwd_h_b<false>, nb - n_done, 32 * HB_WAVES, HB_THREADS, ldsh, ts, n_done);
        }, whole_rounds);
    }
    case HidKernel::T: {
        ProfScope ps("k_mvn_enc_bwd_h_t", st);
        return launch_lds(k_mvn_enc_bwd_h_t, dim3((unsigned)((nb + BH_P - 1) / BH_P)), dim3(BH_THREADS), bh_lds_bytes(dm.D), st, dm,
                          c.cfg->scale, a.packws + c.pk.wpT, c.gtab, a.h, a.eps, a.ldT, a.gxT, c.gdT,
                          rt.f1t ? (float*)nullptr : c.ghpre, a.hT, rt.f1t ? c.ghpre : (float*)nullptr);
    }
    case HidKernel::P:
        return launch_lds(k_mvn_enc_bwd_h_p, grid_p, dim3(ENC_THREADS), enc_bwdh_p_lds_floats(dm.D) * sizeof(float), st, dm,
                          c.cfg->scale, a.packws, c.gtab, a.h, a.eps, a.ldT, a.gx, c.ghpre);
    case HidKernel::Fast:
        return launch_lds(k_mvn_enc_bwd_h_fast, grid_p, dim3(ENC_THREADS), enc_bwdh_fast_lds_floats(dm.D) * sizeof(float), st, dm,
                          c.cfg->scale, a.W21, a.W22, a.h, a.eps, a.ldT, a.gx, c.ghpre);
    case HidKernel::Generic:
        return with_hidden_width(dm.Hp, [&](auto ht) -> int {
            return launch_lds(k_mvn_enc_bwd_h<decltype(ht)::value>, grid_p, dim3(ENC_THREADS),
                              enc_bwdh_lds_floats(dm.D, dm.Hp) * sizeof(float), st, dm, c.cfg->scale, a.W21, a.W22, a.h, a.eps, a.ldT,
                              a.gx, c.ghpre);
        });
    case HidKernel::None: break;
    }
    return VX_OK;
}

// Stage 2, the head weight gradient on stream ws (the launch stream, or for WgtKernel::B of a pair the side stream):
// slabs_w[n_prw][.] over a grid of n_rowslabs x n_prw, with what has to precede it on that stream
static int bwd_weights(const BwdCtx& c, hipStream_t ws) {
    const BwdArgs& a = c.a; const BwdRoute& rt = c.rt; const EncDims& dm = c.dm;
    const int64_t nb = a.nb, Rp = c.pk.Rp, H = c.cfg->H;
    const dim3 grid((unsigned)rt.n_rowslabs, (unsigned)rt.n_prw);
    switch (rt.wgt) {
    case WgtKernel::B: {
        if (rt.split_hs) {                       // bit 1: the forward call already wrote the fp16 terms of hT here
            hipLaunchKernelGGL(k_split2_f16, dim3(num_cu() * 8), dim3(256), 0, ws, a.hT, nb * 64, a.packws + c.pk.hscale, c.hs3);
            VX_CHECK_LAUNCH();
        }
        if (rt.absmax) {                         // the operand maxima, normally collected by k_mvn_enc_bwd_h_b
            hipLaunchKernelGGL(k_clear_words, dim3(1), dim3(64), 0, ws, c.maxw, 4);
            hipLaunchKernelGGL(k_absmax3, dim3(grid_1d(nb * dm.D, 1024)), dim3(256), 0, ws, a.gxT, (const float*)c.gdT, a.epsT,
                               nb * dm.D, c.maxw);
            VX_CHECK_LAUNCH();
        }
        // (its own bracket on ITS stream beside the hidden gradient: the kernel's span while it shares the chip with it)
        ProfScope ps(ws == c.st ? "k_mvn_enc_bwd_w_b" : "k_mvn_enc_bwd_w_b beside k_mvn_enc_bwd_h_b2", ws);
        // (two full-size tile buffers: the three-buffer form of k_mvn_bwd_b.hip measured no faster -- docs/NOTEBOOK.md, round 5)
        return launch_lds(k_mvn_enc_bwd_w_b<2>, grid, dim3(BWB_THREADS), bb_lds_bytes(dm.D), ws, dm, (const uint16_t*)c.hs3, a.epsT,
                          (const float*)c.gdT, a.gxT, c.gtab, c.sc, (const uint32_t*)c.maxw, c.slabs_w, Rp * (H + 1));
    }
    case WgtKernel::T_fc1: {
        const int n_jg1 = (int)((dm.J + 127) / 128), n_prf = c.p.n_prf;
        size_t lds = bt_lds_bytes(dm.D);
        const size_t ldsf = fc1_bwd_lds_floats(dm.Hp) * sizeof(float);
        if (ldsf > lds) lds = ldsf;
        ProfScope ps("k_mvn_enc_bwd_w_t + k_fc1_bwd", ws);
        return launch_lds(k_bwd_wt_fc1, dim3((unsigned)(rt.n_rowslabs * rt.n_prw + n_jg1 * n_prf)), dim3(BT_THREADS), lds, ws, dm, a.hT,
                          a.epsT, (const float*)c.gdT, a.gxT, c.gtab, c.slabs_w, Rp * (H + 1), rt.n_rowslabs, rt.n_prw, a.y, a.rows,
                          (const float*)c.ghpre, c.slabs_f, c.p.lenf, f1fast_ok(c.cfg, c.ghpre, a.y), n_jg1, n_prf);
    }
    case WgtKernel::T: {
        ProfScope ps("k_mvn_enc_bwd_w_t", ws);
        return launch_lds(k_mvn_enc_bwd_w_t, grid, dim3(BT_THREADS), bt_lds_bytes(dm.D), ws, dm, a.hT, a.epsT, c.gdT, a.gxT, c.gtab,
                          c.slabs_w, Rp * (H + 1));
    }
    case WgtKernel::FastPacked: case WgtKernel::Fast: {
        const bool pk = rt.wgt == WgtKernel::FastPacked;       // packed rows through gtab | the reference row order
        return launch_lds(pk ? k_mvn_enc_bwd_w_fast<true> : k_mvn_enc_bwd_w_fast<false>, grid, dim3(ENC_THREADS),
                          enc_bwdw_fast_lds_floats(dm.D) * sizeof(float), ws, dm, c.cfg->scale, a.h, a.eps, a.ldT, a.gx,
                          pk ? c.gtab : (const uint32_t*)nullptr, c.slabs_w, pk ? Rp * (H + 1) : c.p.lenw);
    }
    case WgtKernel::Generic:
        return with_hidden_width(dm.Hp, [&](auto ht) -> int {
            return launch_lds(k_mvn_enc_bwd_w<decltype(ht)::value>, grid, dim3(ENC_THREADS), enc_bwdw_lds_floats(dm.D, dm.Hp) * sizeof(float),
                              ws, dm, c.cfg->scale, a.h, a.eps, a.ldT, a.gx, c.slabs_w, c.p.lenw);
        });
    case WgtKernel::None: break;
    }
    return VX_OK;
}

// Stage 3, the fc1 weight gradient on stream fs: slabs_f[n_prf][lenf] from ghpre (or ghpreT) and the responses
static int bwd_fc1(const BwdCtx& c, hipStream_t fs) {
    const BwdArgs& a = c.a; const EncDims& dm = c.dm;
    const int n_prf = c.p.n_prf;
    const int64_t lenf = c.p.lenf;
    switch (c.rt.fc1) {
    case Fc1Kernel::C: {
        // from dimension-major operands through LDS (k_fc1_bwd_c.hip; ghpre holds ghpreT): two fp16 terms of ghpre when the
        // hidden-gradient kernel collected the step's largest |ghpre| (maxw[3]), three bf16 terms otherwise
        ProfScope ps("k_fc1_bwd_c", fs);
        return launch_lds(c.rt.maxw_ready ? k_fc1_bwd_c<true> : k_fc1_bwd_c<false>, dim3((unsigned)((dm.J + 1 + 511) / 512), (unsigned)n_prf),
                          dim3(F1C_THREADS), f1c_lds_bytes(), fs, dm, a.yT, a.yT_stride, c.ghpre, c.slabs_f, lenf,
                          c.rt.maxw_ready ? (const uint32_t*)c.maxw : (const uint32_t*)nullptr);
    }
    case Fc1Kernel::T:
        return launch_lds(k_fc1_bwd_t, dim3((unsigned)((dm.J + 511) / 512), (unsigned)n_prf), dim3(F1_THREADS), f1_lds_bytes(dm.J), fs, dm,
                          a.yT, a.yT_stride, c.ghpre, c.slabs_f, lenf);
    case Fc1Kernel::Small: case Fc1Kernel::Wide:
        return fc1_bwd_person_major(dm, c.rt.fc1 == Fc1Kernel::Small, c.p.n_jg, n_prf, a.y, a.rows, c.ghpre, c.slabs_f, lenf,
                                    f1fast_ok(c.cfg, c.ghpre, a.y), fs);
    case Fc1Kernel::Rode: break;                           // launched with the head weight gradient: its slabs are summed by the tail
    case Fc1Kernel::None:                                  // nb == 0: no kernel wrote a slab
        if (hipError_t he = hipMemsetAsync(c.slabs_w, 0, sizeof(float) * (size_t)(c.rt.n_prw * c.p.lenw + n_prf * lenf), fs)) return (int)he;
    }
    return VX_OK;
}

// Stage 4, the tail: the slabs summed into genc, the loss.  Flat encoder-gradient layout = nn.Linear order:
// [W1 | b1 | W21 | b21 | W22 | b22]; loss grads = -dELBO.  f1_done: the side stream already summed the fc1 slabs into genc
static int bwd_tail(const BwdCtx& c, bool f1_done) {
    const BwdArgs& a = c.a;
    const LossTail* tail = a.tail;
    const int64_t nb = a.nb, Rp = c.pk.Rp, H = c.cfg->H, lenf = c.p.lenf;
    const int n_prf = c.p.n_prf;
    void* hs = (void*)c.st;
    uint32_t* step_dev = const_cast<uint32_t*>(c.cfg->step_dev);
    int rc;
    if (c.rt.packed) {
        // ONE launch ends the call (k_enc_bwd_tail): the head gradients back in the reference layout, the fc1 slabs summed
        // (unless the side stream did), the loss of a small batch -- three launches of ~5 us until round 5
        const int n_unpack = (int)((Rp + 3) / 4);
        const int n_f1 = f1_done ? 0 : grid_1d(lenf, 64);
        const bool loss_here = tail && nb <= 4096;
        hipLaunchKernelGGL(k_enc_bwd_tail, dim3((unsigned)(n_unpack + n_f1 + (loss_here ? 1 : 0))), dim3(256), 0, c.st, (int)c.cfg->D, (int)H,
                           c.slabs_w, c.rt.n_prw, Rp * (H + 1), -1.0f, a.genc + lenf, n_unpack, (const float*)c.slabs_f, (int64_t)n_prf, lenf,
                           a.genc, n_f1, loss_here ? tail->ll : nullptr, loss_here ? tail->ent : nullptr, nb,
                           loss_here ? tail->alpha : 0.f, loss_here ? tail->loss : nullptr, loss_here ? tail->sum_ws : nullptr,
                           loss_here ? step_dev : nullptr);
        VX_CHECK_LAUNCH();
        if (tail && !loss_here) return vx_sum2(tail->ll, tail->ent, nb, tail->alpha, tail->loss, tail->sum_ws, step_dev, hs);
        return VX_OK;
    }
    if (!f1_done) {
        rc = vx_reduce_slabs(c.slabs_f, n_prf, lenf, -1.0f, a.genc, hs);
        if (rc) return rc;
    }
    rc = vx_reduce_slabs(c.slabs_w, c.rt.n_prw, c.p.lenw_ref, -1.0f, a.genc + lenf, hs);
    if (rc) return rc;
    if (tail) return vx_sum2(tail->ll, tail->ent, nb, tail->alpha, tail->loss, tail->sum_ws, step_dev, hs);
    return VX_OK;
}

// vx_mvn_enc_backward(_loss): check the arguments, resolve the route, refuse, then the four stages in order.  The only state
// carried across stages is what a fork's success decides at run time: w_done (the head weight gradient already runs on
// stream 1) and f1_done (the fc1 gradient ran and was summed on stream 0).
static int mvn_enc_backward_impl(const vx_irt_cfg* cfg, const BwdArgs& a, void* hs) {
    if (!enc_cfg_ok(cfg) || !a.y || !a.W21 || !a.W22 || !a.h || !a.eps || !a.ldT || (!a.gx && !a.gxT) || !a.genc || !a.workspace ||
        a.nb < 0)
        return VX_EINVAL;
    const MvnPlan p = mvn_plan(cfg, a.nb);
    const BwdRoute rt = bwd_route(cfg, p, a);
    if (rt.refused) return VX_EINVAL;
    hipStream_t st = (hipStream_t)hs;
    const BwdCtx c = bwd_ctx(cfg, a, p, rt, st);
    int rc;
    bool w_done = false, f1_done = false;
    ForkScope f1_fork, w_fork;                             // joined below, or by the scope on an error return
    std::optional<ProfScope> pair_ps;
    if (rt.gd_first) {                                     // (bit 0: the likelihood's last pass made gdT)
        hipLaunchKernelGGL(k_mvn_gd, dim3(num_cu() * 8), dim3(256), 0, st, (const float4*)a.gxT, (const float4*)a.epsT,
                           (const float4*)a.ldT, cfg->scale, a.nb * cfg->D / 4, (float4*)c.gdT);
        VX_CHECK_LAUNCH();
    }
    if (rt.packed) {
        // the bracket of the PAIR on the launch stream: from in front of the fork to behind the join of the head weight gradient's
        // stream = the span of {hidden gradient | head weight gradient} side by side (what bench.py prices with the sum of the two
        // kernels' flops); dropped at once when the two do not run side by side
        pair_ps.emplace("k_mvn_enc_bwd_h_b2 | k_mvn_enc_bwd_w_b side by side", st);
        if (rt.pair && w_fork.fork(side_stream(1, st), st)) {
            // The head weight gradient needs nothing the hidden gradient makes once the step's operand maxima are there (bit 2:
            // vx_irt_lik_grad collected them): it starts NOW on a second stream, and the hidden gradient and then the fc1
            // gradient run beside it on the launch stream.  The two large kernels each fill the chip alone; side by side
            // their workgroups interleave and neither leaves CUs idle in its last round or behind its barriers: 5.2 -> 4.7 ms
            // for the backward phase of the 1M step.  (The hidden-gradient kernels still add their waves' maxima to the same
            // words: values that are already there, so the words do not change under the reader.)
            // (launched before or behind the hidden gradient: 9.63 against 9.62 ms -- the order does not matter)
            w_done = true;
            rc = bwd_weights(c, w_fork.side());
            if (rc) return rc;
        } else {
            pair_ps->cancel();                                 // one kernel after the other: each has a bracket of its own
        }
    }
    rc = bwd_hidden(c, w_done);
    if (rc) return rc;
    if (rt.fc1_side && f1_fork.fork(side_stream(0, st), st)) {
        // the fc1 weight gradient needs ghpre only: it runs on a second stream beside the head weight gradient below
        // (0.33 ms of a 1M step that used to follow it) and is joined before this call returns (also on an error return)
        rc = bwd_fc1(c, f1_fork.side());
        if (rc) return rc;
        rc = vx_reduce_slabs(c.slabs_f, p.n_prf, p.lenf, -1.0f, a.genc, (void*)f1_fork.side());
        if (rc) return rc;
        f1_done = true;
    }
    if (w_done) {
        rc = w_fork.join();
        if (rc) return rc;
        pair_ps.reset();                                   // the launch stream is behind both kernels here
    } else {
        rc = bwd_weights(c, st);
        if (rc) return rc;
    }
    if (f1_done) {
        rc = f1_fork.join();                               // the fc1 gradient is in genc
        if (rc) return rc;
    } else {
        rc = bwd_fc1(c, st);
        if (rc) return rc;
    }
    return bwd_tail(c, f1_done);
}

int vx_mvn_enc_backward(const vx_irt_cfg* cfg, const uint8_t* y, const int64_t* rows, int64_t nb,
                        const float* W21, const float* W22, const float* h, const float* eps, const float* ldT,
                        const float* gx, const float* hT, const float* epsT, const float* gxT, const uint8_t* yT,
                        int64_t yT_stride, float* genc, float* workspace, const float* packws, int32_t gd_ready, void* hs) {
    return mvn_enc_backward_impl(cfg, BwdArgs{y, rows, nb, W21, W22, h, eps, ldT, gx, hT, epsT, gxT, yT, yT_stride, genc, workspace,
                                              packws, gd_ready, nullptr}, hs);
}

int vx_mvn_enc_backward_loss(const vx_irt_cfg* cfg, const uint8_t* y, const int64_t* rows, int64_t nb,
                             const float* W21, const float* W22, const float* h, const float* eps, const float* ldT,
                             const float* gx, const float* hT, const float* epsT, const float* gxT, const uint8_t* yT,
                             int64_t yT_stride, float* genc, float* workspace, const float* packws, int32_t gd_ready,
                             const float* ll, const float* ent, float loss_alpha, float* loss, float* sum_workspace, void* hs) {
    if (!ll || !ent || !loss || !sum_workspace) return VX_EINVAL;
    const LossTail tail{ll, ent, loss_alpha, loss, sum_workspace};
    return mvn_enc_backward_impl(cfg, BwdArgs{y, rows, nb, W21, W22, h, eps, ldT, gx, hT, epsT, gxT, yT, yT_stride, genc, workspace,
                                              packws, gd_ready, &tail}, hs);
}

// ------------------------------------------------------------------------------------------------
// J <= I1_PERSON_LANES_MAX_J: the person-per-lane kernel (k_irt1d); above it the item-per-lane kernel (k_irt1d_items) -- see
// the measurements at the head of k_irt1d_items
#define I1_PERSON_LANES_MAX_J 256
static int irt1d_blocks(int64_t nb, int J) {
    int64_t blocks, cap;
    if (J <= I1_PERSON_LANES_MAX_J) {
        // a workgroup takes chunks of 64 persons: one chunk each while they all fit the chip together (eight workgroups a
        // CU), strided chunks beyond that -- the slabs a block writes are summed by one small kernel either way
        blocks = (nb + 63) / 64;
        cap = (int64_t)num_cu() * 8;
    } else {
        const int64_t g = i1_group_size(nb, (int64_t)num_cu() * 4 * (I1_THREADS / 64));
        const int64_t n_groups = (nb + g - 1) / g;                     // a wave walks groups of up to 64 persons
        blocks = (n_groups + 3) / 4;
        cap = (int64_t)num_cu() * 4;
    }
    if (blocks > cap) blocks = cap;
    return (int)(blocks < 1 ? 1 : blocks);
}

static bool irt1d_cfg_ok(const vx_irt_cfg* cfg) {
    return cfg && cfg->D == 1 && cfg->J >= 1 && cfg->J <= 1024 && cfg->model >= VX_IRT_1PL &&
           cfg->model <= VX_IRT_4PL;
}

int64_t vx_irt1d_workspace_floats(const vx_irt_cfg* cfg, int64_t nb) {
    if (!irt1d_cfg_ok(cfg) || nb < 0) return VX_EINVAL;
    return (int64_t)irt1d_blocks(nb, cfg->J) * (4 * cfg->J + 1) + 4;    // the slabs | Adam's count of the step (k_reduce_adam)
}

static int irt1d_grad_impl(const vx_irt_cfg* cfg, const uint8_t* y, const int64_t* rows, int64_t nb, int64_t gid0,
                  const float* loc, const float* raw, const float* eps_in, const float* a, const float* b,
                  const float* c_un, const float* d_un, float* gloc, float* graw, float* elbo, float* gitem,
                  float* loss, uint32_t* step_dev, float* workspace, void* hs, const vx_adam_tail* opt) {
    if (!irt1d_cfg_ok(cfg) || !y || !loc || !raw || !b || !gloc || !graw || !elbo || !gitem || !workspace || nb < 0)
        return VX_EINVAL;
    if (cfg->model >= VX_IRT_2PL && !a) return VX_EINVAL;
    if (cfg->model >= VX_IRT_3PL && !c_un) return VX_EINVAL;
    if (cfg->model == VX_IRT_4PL && !d_un) return VX_EINVAL;
    const int blocks = irt1d_blocks(nb, cfg->J);
    Irt1dDims dm;
    dm.J = cfg->J; dm.model = cfg->model; dm.Dc = cfg->Dc; dm.scale = cfg->scale; dm.nb = nb;
    dm.gsz = i1_group_size(nb, (int64_t)num_cu() * 4 * (I1_THREADS / 64));
    const bool by_person = cfg->J <= I1_PERSON_LANES_MAX_J;
    // person-per-lane: item table, item sums, parked terms; item-per-lane: one partial slot per wave
    const size_t lds = by_person ? i1_lds_bytes(cfg->J, cfg->model) : sizeof(float) * 4 * (size_t)cfg->J * (I1_THREADS / 64);
    hipStream_t st = (hipStream_t)hs;
    const int words_ok = (cfg->J % 4 == 0 && aligned16(y)) ? 1 : 0;     // 4-byte response loads need aligned rows
    const int wpl_need = (cfg->J + 255) / 256;
    int rc = VX_EINVAL;
#define LAUNCH_1DK(KERNEL)                                                                                    \
    rc = set_lds(KERNEL, lds);                                                                                \
    if (rc) return rc;                                                                                        \
    hipLaunchKernelGGL(KERNEL, dim3(blocks), dim3(I1_THREADS), lds, st, dm, y, rows, gid0, loc, raw, eps_in, cfg->seed, \
                       cfg->step, step_dev, cfg->stream, a, b, c_un, d_un, gloc, graw, elbo, workspace)
#define LAUNCH_1DW(MODEL, WORDS)                                                                              \
    if (by_person) { LAUNCH_1DK((k_irt1d<MODEL, WORDS>)); }                                                   \
    else if (wpl_need <= 1) { LAUNCH_1DK((k_irt1d_items<MODEL, 1, WORDS>)); }                                 \
    else if (wpl_need <= 2) { LAUNCH_1DK((k_irt1d_items<MODEL, 2, WORDS>)); }                                 \
    else { LAUNCH_1DK((k_irt1d_items<MODEL, 4, WORDS>)); }
#define LAUNCH_1D(MODEL)                                           \
    if (words_ok) { LAUNCH_1DW(MODEL, true) } else { LAUNCH_1DW(MODEL, false) }
    switch (cfg->model) {
        case VX_IRT_1PL: LAUNCH_1D(1) break;
        case VX_IRT_2PL: LAUNCH_1D(2) break;
        case VX_IRT_3PL: LAUNCH_1D(3) break;
        default: LAUNCH_1D(4) break;
    }
#undef LAUNCH_1D
#undef LAUNCH_1DW
#undef LAUNCH_1DK
    VX_CHECK_LAUNCH();
    return reduce_step_slabs(workspace, blocks, cfg->J, gitem, loss, step_dev, hs, opt);
}

int vx_irt1d_grad(const vx_irt_cfg* cfg, const uint8_t* y, const int64_t* rows, int64_t nb, int64_t gid0,
                  const float* loc, const float* raw, const float* eps_in, const float* a, const float* b,
                  const float* c_un, const float* d_un, float* gloc, float* graw, float* elbo, float* gitem,
                  float* loss, uint32_t* step_dev, float* workspace, void* hs) {
    return irt1d_grad_impl(cfg, y, rows, nb, gid0, loc, raw, eps_in, a, b, c_un, d_un, gloc, graw, elbo, gitem, loss, step_dev,
                           workspace, hs, nullptr);
}

int vx_irt1d_grad_adam(const vx_irt_cfg* cfg, const uint8_t* y, const int64_t* rows, int64_t nb, int64_t gid0,
                       const float* loc, const float* raw, const float* eps_in, const float* a, const float* b,
                       const float* c_un, const float* d_un, float* gloc, float* graw, float* elbo, float* gitem,
                       float* loss, uint32_t* step_dev, float* workspace, const vx_adam_tail* opt, void* hs) {
    if (!opt || !loss) return VX_EINVAL;
    return irt1d_grad_impl(cfg, y, rows, nb, gid0, loc, raw, eps_in, a, b, c_un, d_un, gloc, graw, elbo, gitem, loss, step_dev,
                           workspace, hs, opt);
}

int vx_irt1d_score_grad(int64_t nb, float scale, const float* elbo, const float* eps, const float* raw, const int64_t* rows,
                        float* baseline, float base_beta, int32_t base_by_row, float* log_r, float* gloc, float* graw,
                        void* hs) {
    if (nb < 0 || !elbo || !eps || !raw || !gloc || !graw) return VX_EINVAL;
    if (nb == 0) return VX_OK;
    hipLaunchKernelGGL(k_irt1d_score, dim3(grid_1d(nb, 256)), dim3(256), 0, (hipStream_t)hs, nb, scale, elbo, eps, raw, rows,
                       baseline, base_beta, (int)base_by_row, log_r, gloc, graw);
    VX_CHECK_LAUNCH();
    return VX_OK;
}

// ---- score-function operands of the multivariate Normal guides (k_mvn_score.hip)
int vx_mvn_score_operands(const vx_irt_cfg* cfg, int64_t nb, const int64_t* rows, int32_t kind, const float* h,
                          const float* W22, const float* b22, const float* M, const float* eps, const float* ll,
                          const float* ent, float* baseline, float base_beta, int32_t base_by_row, float* log_r, float* w,
                          float* gx, float* gxT, float* gdT, void* hs) {
    if (!cfg || cfg->D < 2 || cfg->D > 127 || nb < 0 || kind < 0 || kind > 2 || !eps || !ll || !ent || (!gx && !gxT && !w))
        return VX_EINVAL;
    if (kind == 0 && (!h || !W22 || !b22 || cfg->H < 1)) return VX_EINVAL;
    if (kind != 0 && !M) return VX_EINVAL;
    if (nb == 0) return VX_OK;
    const size_t lds = ms_lds_bytes(cfg->D, cfg->H, kind);
    if (lds > 160 * 1024) return VX_EINVAL;
    const dim3 grid((unsigned)((nb + MS_THREADS - 1) / MS_THREADS));
    hipStream_t st = (hipStream_t)hs;
    int rc;
#define LAUNCH_MS(K)                                                                                               \
    rc = set_lds(k_mvn_score_operands<K>, lds);                                                                    \
    if (rc) return rc;                                                                                             \
    hipLaunchKernelGGL(k_mvn_score_operands<K>, grid, dim3(MS_THREADS), lds, st, (int)cfg->D, (int)cfg->H, nb,     \
                       cfg->scale, rows, h, W22, b22, M, eps, ll, ent, baseline, base_beta, (int)base_by_row, log_r, w, gx, gxT, gdT)
    if (kind == 0) { LAUNCH_MS(0); } else if (kind == 1) { LAUNCH_MS(1); } else { LAUNCH_MS(2); }
#undef LAUNCH_MS
    VX_CHECK_LAUNCH();
    return VX_OK;
}

// the MFMA form of kind 0 (k_mvn_score_b.hip): the shapes whose forward ran on the f16x2 kernels
static bool score_heads_shape(const vx_irt_cfg* cfg) {
    return cfg && !force_generic() && fwb_shape(cfg) && cfg->H == 64 && cfg->D % 4 == 0 && cfg->D >= 8 && cfg->D <= 124 &&
           sb_lds_bytes(cfg->D) <= 160 * 1024;
}
int64_t vx_mvn_score_heads_workspace_floats(const vx_irt_cfg* cfg) {
    if (!score_heads_shape(cfg)) return VX_EINVAL;
    return sb_img_floats(cfg->D);
}
int vx_mvn_score_heads(const vx_irt_cfg* cfg, int64_t nb, const int64_t* rows, const float* h, const float* W22, const float* b22,
                       const float* packws, const float* eps, const float* ll, const float* ent,
                       float* baseline, float base_beta, int32_t base_by_row, float* log_r, float* gxT, float* gdT,
                       float* workspace, void* hs) {
    if (!score_heads_shape(cfg) || nb < 0 || !h || !W22 || !b22 || !packws || !eps || !ll || !ent || !gxT || !workspace ||
        !aligned16(h) || !aligned16(eps) || !aligned16(workspace))
        return VX_EINVAL;
    if (nb == 0) return VX_OK;
    const float* sc = packws + pack_layout(cfg).sc;
    hipStream_t st = (hipStream_t)hs;
    const int D = cfg->D;
    hipLaunchKernelGGL(k_pack_heads_col, dim3((unsigned)sb_tiles(D)), dim3(256), 0, st, D, W22, b22, sc, (uint8_t*)workspace);
    VX_CHECK_LAUNCH();
    // a batch that fills the chip: one workgroup of eight consumer waves and a loader wave a CU, the tiles through LDS once
    // (the L2 serves the 2 MB image to every wave of the plain form at 22 TB/s: rule 30); a smaller one: the plain form
    const bool ring = seams().score_ring && nb >= 16384 && sbr_lds_bytes(D) <= 160 * 1024;
    int rc;
    ProfScope ps("k_mvn_score_b", st, nb);
    if (ring) {
        const size_t lds = sbr_lds_bytes(D);
        rc = set_lds(k_mvn_score_b<true>, lds);
        if (rc) return rc;
        hipLaunchKernelGGL(k_mvn_score_b<true>, dim3((unsigned)((nb + SBR_CONSUMERS * SB_WP - 1) / (SBR_CONSUMERS * SB_WP))),
                           dim3(SBR_THREADS), lds, st, D, nb, cfg->scale, rows, h, (const uint8_t*)workspace, sc, eps, ll, ent, baseline,
                           base_beta, (int)base_by_row, log_r, gxT, gdT);
    } else {
        const size_t lds = sb_lds_bytes(D);
        rc = set_lds(k_mvn_score_b<false>, lds);
        if (rc) return rc;
        hipLaunchKernelGGL(k_mvn_score_b<false>, dim3((unsigned)((nb + SB_WAVES * SB_WP - 1) / (SB_WAVES * SB_WP))), dim3(SB_THREADS), lds,
                           st, D, nb, cfg->scale, rows, h, (const uint8_t*)workspace, sc, eps, ll, ent, baseline, base_beta,
                           (int)base_by_row, log_r, gxT, gdT);
    }
    VX_CHECK_LAUNCH();
    return VX_OK;
}

int vx_mvn_score_diag(const vx_irt_cfg* cfg, int64_t nb, const int64_t* rows, const float* w, int32_t shared, float* gM,
                      void* hs) {
    if (!cfg || cfg->D < 2 || cfg->D > 127 || nb < 0 || !w || !gM) return VX_EINVAL;
    if (nb == 0) return VX_OK;
    const unsigned blocks = shared ? 1u : (unsigned)grid_1d(nb * cfg->D, 256);
    hipLaunchKernelGGL(k_mvn_score_diag, dim3(blocks), dim3(256), 0, (hipStream_t)hs, (int)cfg->D, nb, rows, w, (int)shared, gM);
    VX_CHECK_LAUNCH();
    return VX_OK;
}

// ---- D = 1 on the host-compacted lists of observed cells (k_irt1d_sparse.hip); full batch only
static int irt1d_sp_blocks(int64_t n_groups) {
    int64_t blocks = (n_groups + SP_THREADS / 64 - 1) / (SP_THREADS / 64);
    if (blocks > (int64_t)num_cu() * 4) blocks = (int64_t)num_cu() * 4;
    return (int)(blocks < 1 ? 1 : blocks);
}

int64_t vx_irt1d_sparse_workspace_floats(const vx_irt_cfg* cfg, int64_t n_groups) {
    if (!irt1d_cfg_ok(cfg) || n_groups < 0) return VX_EINVAL;
    return (int64_t)irt1d_sp_blocks(n_groups) * (4 * cfg->J + 1) + 4;                      // one slab per block | Adam's count
}

static int irt1d_sparse_grad_impl(const vx_irt_cfg* cfg, const uint16_t* pent, const int32_t* glen, int32_t Lq,
                         const int32_t* pidx, int64_t n_groups, int64_t gid0, const float* loc, const float* raw,
                         const float* eps_in, const float* a, const float* b, const float* c_un, const float* d_un,
                         float* gloc, float* graw, float* elbo, float* gitem, float* loss, uint32_t* step_dev,
                         float* workspace, void* hs, const vx_adam_tail* opt) {
    if (!irt1d_cfg_ok(cfg) || !pent || !glen || !pidx || Lq < 0 || !loc || !raw || !b || !gloc || !graw || !elbo ||
        !gitem || !workspace || n_groups < 0 || cfg->J > 32767)
        return VX_EINVAL;
    if (cfg->model >= VX_IRT_2PL && !a) return VX_EINVAL;
    if (cfg->model >= VX_IRT_3PL && !c_un) return VX_EINVAL;
    if (cfg->model == VX_IRT_4PL && !d_un) return VX_EINVAL;
    const int blocks = irt1d_sp_blocks(n_groups);
    // every |t| <= 1, so a block's integer sums stay below 2^30 whatever the data: persons a block can see x scale
    const int64_t n_waves = (int64_t)blocks * (SP_THREADS / 64);
    const int64_t per_block = ((n_groups + n_waves - 1) / n_waves) * SP_THREADS;
    float sb = 1048576.0f;                                                                 // 2^20
    while (sb * (float)(per_block > 0 ? per_block : 1) > 1073741824.0f) sb *= 0.5f;
    Irt1dSpDims dm;
    dm.J = cfg->J; dm.model = cfg->model; dm.Lq = Lq; dm.Dc = cfg->Dc; dm.scale = cfg->scale;
    dm.sb = sb; dm.inv_sb = 1.0f / sb; dm.n_groups = n_groups;
    hipStream_t st = (hipStream_t)hs;
    const size_t lds = (size_t)cfg->J * (cfg->model >= VX_IRT_3PL ? 52 : 24);
    int rc = VX_EINVAL;
#define LAUNCH_SP(MODEL)                                                                                      \
    rc = set_lds(k_irt1d_sp<MODEL>, lds);                                                                     \
    if (rc) return rc;                                                                                        \
    hipLaunchKernelGGL((k_irt1d_sp<MODEL>), dim3((unsigned)blocks), dim3(SP_THREADS), lds, st, dm, (const uint2*)pent, glen, \
                       pidx, gid0, loc, raw, eps_in, cfg->seed, cfg->step, step_dev, cfg->stream, a, b, c_un, d_un, gloc,   \
                       graw, elbo, workspace)
    switch (cfg->model) {
        case VX_IRT_1PL: LAUNCH_SP(1); break;
        case VX_IRT_2PL: LAUNCH_SP(2); break;
        case VX_IRT_3PL: LAUNCH_SP(3); break;
        default: LAUNCH_SP(4); break;
    }
#undef LAUNCH_SP
    VX_CHECK_LAUNCH();
    return reduce_step_slabs(workspace, blocks, cfg->J, gitem, loss, step_dev, hs, opt);
}

int vx_irt1d_sparse_grad(const vx_irt_cfg* cfg, const uint16_t* pent, const int32_t* glen, int32_t Lq,
                         const int32_t* pidx, int64_t n_groups, int64_t gid0, const float* loc, const float* raw,
                         const float* eps_in, const float* a, const float* b, const float* c_un, const float* d_un,
                         float* gloc, float* graw, float* elbo, float* gitem, float* loss, uint32_t* step_dev,
                         float* workspace, void* hs) {
    return irt1d_sparse_grad_impl(cfg, pent, glen, Lq, pidx, n_groups, gid0, loc, raw, eps_in, a, b, c_un, d_un, gloc, graw, elbo,
                                  gitem, loss, step_dev, workspace, hs, nullptr);
}

int vx_irt1d_sparse_grad_adam(const vx_irt_cfg* cfg, const uint16_t* pent, const int32_t* glen, int32_t Lq,
                              const int32_t* pidx, int64_t n_groups, int64_t gid0, const float* loc, const float* raw,
                              const float* eps_in, const float* a, const float* b, const float* c_un, const float* d_un,
                              float* gloc, float* graw, float* elbo, float* gitem, float* loss, uint32_t* step_dev,
                              float* workspace, const vx_adam_tail* opt, void* hs) {
    if (!opt || !loss) return VX_EINVAL;
    return irt1d_sparse_grad_impl(cfg, pent, glen, Lq, pidx, n_groups, gid0, loc, raw, eps_in, a, b, c_un, d_un, gloc, graw, elbo,
                                  gitem, loss, step_dev, workspace, hs, opt);
}

// ------------------------------------------------------------------------------------------------
int vx_mvn_bbvi_forward(const vx_irt_cfg* cfg, int64_t nb, const int64_t* rows, int64_t gid0, const float* loc,
                        const float* M, int32_t shared, const float* eps_in, float* x, float* eps, float* ent,
                        void* hs) {
    if (!cfg || cfg->D < 2 || cfg->D > 128 || !loc || !M || !x || !eps || !ent || nb < 0) return VX_EINVAL;
    if (nb == 0) return VX_OK;
    int64_t blocks = (nb + 3) / 4;
    if (blocks > (int64_t)num_cu() * 8) blocks = (int64_t)num_cu() * 8;
    hipLaunchKernelGGL(k_mvn_bbvi_fwd, dim3((unsigned)blocks), dim3(BB_THREADS), 0, (hipStream_t)hs, (int)cfg->D, nb, rows,
                       gid0, loc, M, (int)shared, eps_in, cfg->seed, cfg->step, cfg->stream, x, eps, ent, cfg->step_dev);
    VX_CHECK_LAUNCH();
    return VX_OK;
}

static int bbvi_shared_blocks(int64_t nb) {
    int64_t blocks = (nb + 3) / 4;
    if (blocks > 64) blocks = 64;                           // one [D][D] slab each
    return (int)(blocks < 1 ? 1 : blocks);
}

int64_t vx_mvn_bbvi_bwd_workspace_floats(const vx_irt_cfg* cfg, int64_t nb, int32_t shared) {
    if (!cfg || cfg->D < 2 || cfg->D > 128 || nb < 0) return VX_EINVAL;
    return shared ? (int64_t)bbvi_shared_blocks(nb) * cfg->D * cfg->D : 1;
}

int vx_mvn_bbvi_backward(const vx_irt_cfg* cfg, int64_t nb, const int64_t* rows, const float* M, int32_t shared,
                         const float* gx, const float* eps, float* gloc, float* gM, float* workspace, void* hs) {
    if (!cfg || cfg->D < 2 || cfg->D > 128 || !M || !gx || !eps || !gloc || !gM || nb < 0 || (shared && !workspace))
        return VX_EINVAL;
    if (nb == 0) return VX_OK;
    int64_t blocks = (nb + 3) / 4;
    const int64_t cap = shared ? (int64_t)bbvi_shared_blocks(nb) : (int64_t)num_cu() * 8;
    if (blocks > cap) blocks = cap;
    const size_t lds = shared ? sizeof(long long) * (size_t)cfg->D * cfg->D : 0;
    int rc = set_lds(k_mvn_bbvi_bwd, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(k_mvn_bbvi_bwd, dim3((unsigned)blocks), dim3(BB_THREADS), lds, (hipStream_t)hs, (int)cfg->D, nb,
                       cfg->scale, rows, M, (int)shared, gx, eps, gloc, shared ? workspace : gM);
    VX_CHECK_LAUNCH();
    if (shared) return vx_reduce_slabs(workspace, blocks, (int64_t)cfg->D * cfg->D, 1.0f, gM, hs);   // fixed-order sum of the slabs
    return VX_OK;
}

// ------------------------------------------------------------------------------------------------
static bool nenc_cfg_ok(const vx_irt_cfg* cfg) { return cfg && cfg->H >= 1 && cfg->H <= 128 && cfg->J >= 1; }

static void nenc_plan(const vx_irt_cfg* cfg, int64_t nb, int& nblk, int& n_jg, int& n_prf) {
    int hp = 1;
    while (hp < cfg->H) hp <<= 1;
    const int ppb = 256 / hp;
    int64_t b = (nb + ppb - 1) / ppb;
    if (b > 1024) b = 1024;
    nblk = (int)(b < 1 ? 1 : b);
    n_jg = (cfg->J + FC1_JG - 1) / FC1_JG;
    const int64_t n_ptiles = (nb + ENC_P - 1) / ENC_P;
    int64_t f = num_cu() / n_jg; if (f < 1) f = 1;
    n_prf = (int)(n_ptiles < f ? n_ptiles : f); if (n_prf < 1) n_prf = 1;
}

int64_t vx_norm_enc_param_floats(const vx_irt_cfg* cfg) {
    if (!nenc_cfg_ok(cfg)) return VX_EINVAL;
    return (int64_t)cfg->H * cfg->J + 3 * (int64_t)cfg->H + 2;
}

// the f16x2 NormEncoder forward (k_norm_enc_fwd_h): hidden_dim 64, whole response words; batches from NH_MIN_PERSONS on (two
// more launches make the weight images: not worth it for a minibatch)
#define NH_MIN_PERSONS 4096
#ifndef NH_NP
#define NH_NP 1
#endif
#ifndef NH_PF
#define NH_PF 3
#endif
static bool nenc_h_shape(const vx_irt_cfg* cfg) {
    return !force_generic() && seams().fwd16 && cfg->H == 64 && cfg->J % 4 == 0 && cfg->J >= 256 &&
           nh_lds_bytes<NH_NP>(cfg->J) <= 160 * 1024;
}
int64_t vx_norm_enc_pack_floats(const vx_irt_cfg* cfg) {
    if (!nenc_cfg_ok(cfg)) return VX_EINVAL;
    return nenc_h_shape(cfg) ? nh_pack_floats(cfg->J) : 0;
}

int vx_norm_enc_forward(const vx_irt_cfg* cfg, const uint8_t* y, const int64_t* rows, int64_t nb, const float* W1,
                        const float* b1, const float* W21, const float* b21, const float* W22, const float* b22,
                        float* h, float* loc, float* raw, float* packws, void* hs) {
    if (!nenc_cfg_ok(cfg) || !y || !W1 || !b1 || !W21 || !b21 || !W22 || !b22 || !h || !loc || !raw || nb < 0)
        return VX_EINVAL;
    if (nb == 0) return VX_OK;
    EncDims dm;
    dm.D = 1; dm.J = cfg->J; dm.H = cfg->H; dm.Hp = (cfg->H + 31) / 32 * 32; dm.DS = 3; dm.T = 1; dm.nb = nb;
    if (packws && nb >= NH_MIN_PERSONS && nenc_h_shape(cfg) && aligned16(packws) && aligned16(y) && aligned16(W1) &&
        aligned16(b1) && aligned16(h)) {
        uint8_t* w1img = (uint8_t*)packws;
        float* sc = packws + fb_w1img_floats(cfg->J);
        float* part = sc + 16;
        const int n_ks = (cfg->J + 15) / 16;
        hipLaunchKernelGGL(k_norm_pack_max, dim3(NH_MAX_BLOCKS), dim3(256), 0, (hipStream_t)hs, (int)cfg->J, W1, part);
        VX_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_norm_pack_w1, dim3((unsigned)n_ks), dim3(256), 0, (hipStream_t)hs, (int)cfg->J, W1, (const float*)part, sc,
                           w1img);
        VX_CHECK_LAUNCH();
        ProfScope ps("k_norm_enc_fwd_h", (hipStream_t)hs);
        return launch_lds(k_norm_enc_fwd_h<NH_NP, NH_PF>, dim3((unsigned)((nb + 127) / 128)), dim3(64 * (4 / NH_NP)), nh_lds_bytes<NH_NP>(cfg->J),
                          (hipStream_t)hs, dm, y, rows, (const uint8_t*)w1img, (const float*)sc, b1, W21, b21, W22, b22, h, loc, raw);
    }
    if (!force_generic() && seams().fwd16 && cfg->H == 64 && cfg->J % 4 == 0 && aligned16(y) && aligned16(W1) &&
        aligned16(b1) && aligned16(h) && nb_lds_bytes(cfg->J) <= 160 * 1024) {
        ProfScope ps("k_norm_enc_fwd_b", (hipStream_t)hs);                // fc1 on the bf16 MFMA, W1 shared by the workgroup
        return launch_lds(k_norm_enc_fwd_b, dim3((unsigned)((nb + NB_WAVES * EP_WP - 1) / (NB_WAVES * EP_WP))), dim3(NB_THREADS),
                          nb_lds_bytes(cfg->J), (hipStream_t)hs, dm, y, rows, W1, b1, W21, b21, W22, b22, h, loc, raw);
    }
    if (!force_generic() && cfg->H == 64 && cfg->J % 4 == 0 && aligned16(y) && aligned16(W1) && aligned16(b1) &&
        aligned16(h) && NE_WAVES * norm_fast_wave_floats(cfg->J) * sizeof(float) <= 160 * 1024) {
        return launch_lds(k_norm_enc_fwd_fast, dim3((unsigned)((nb + NE_WAVES * EP_WP - 1) / (NE_WAVES * EP_WP))), dim3(NE_THREADS),
                          NE_WAVES * norm_fast_wave_floats(cfg->J) * sizeof(float), (hipStream_t)hs, dm, y, rows, W1, b1, W21, b21, W22,
                          b22, h, loc, raw);
    }
    const size_t lds = norm_enc_fwd_lds_floats(dm.Hp) * sizeof(float);
    const dim3 grid((unsigned)((nb + ENC_P - 1) / ENC_P));
    return with_hidden_width(dm.Hp, [&](auto ht) -> int {
        return launch_lds(k_norm_enc_fwd<decltype(ht)::value>, grid, dim3(ENC_THREADS), lds, (hipStream_t)hs, dm, y, rows, W1, b1, W21, b21,
                          W22, b22, h, loc, raw);
    });
}

int64_t vx_norm_enc_bwd_workspace_floats(const vx_irt_cfg* cfg, int64_t nb) {
    if (!nenc_cfg_ok(cfg) || nb < 0) return VX_EINVAL;
    int nblk, n_jg, n_prf;
    nenc_plan(cfg, nb, nblk, n_jg, n_prf);
    const int64_t H = cfg->H, J = cfg->J;
    return nb * H + (int64_t)nblk * (2 * H + 2) + (int64_t)n_prf * (H * J + H) + nb * H + 8;   // ghpre | slabs | ghpreT
}

int vx_norm_enc_backward(const vx_irt_cfg* cfg, const uint8_t* y, const int64_t* rows, int64_t nb, const float* W21,
                         const float* W22, const float* h, const float* gloc, const float* graw, const uint8_t* yT,
                         int64_t yT_stride, float* genc, float* workspace, void* hs) {
    if (!nenc_cfg_ok(cfg) || !y || !W21 || !W22 || !h || !gloc || !graw || !genc || !workspace || nb < 0)
        return VX_EINVAL;
    int nblk, n_jg, n_prf;
    nenc_plan(cfg, nb, nblk, n_jg, n_prf);
    const int64_t H = cfg->H, J = cfg->J;
    const int64_t lenh = 2 * H + 2, lenf = H * J + H;
    float* ghpre = workspace;
    float* slabs_h = ghpre + nb * H;
    float* slabs_f = slabs_h + (int64_t)nblk * lenh;
    hipStream_t st = (hipStream_t)hs;
    hipError_t he = hipMemsetAsync(slabs_h, 0, sizeof(float) * (size_t)(nblk * lenh + (nb == 0 ? n_prf * lenf : 0)), st);
    if (he != hipSuccess) return (int)he;
    int rc;
    if (nb > 0) {
        EncDims dm;
        dm.D = 1; dm.J = cfg->J; dm.H = cfg->H; dm.Hp = (cfg->H + 31) / 32 * 32; dm.DS = 3; dm.T = 1; dm.nb = nb;
        const bool tmajor = !force_generic() && yT && !rows && cfg->H == 64 && nb % 4 == 0 && yT_stride % 16 == 0 &&
                            yT_stride >= nb && aligned16(yT) && cfg->J >= 32 && aligned16(workspace) &&
                            f1_lds_bytes(cfg->J) <= 160 * 1024;
        if (tmajor) {
            // dimension-major fc1 gradient (k_fc1_bwd_b / k_fc1_bwd_t): ghpreT lives behind the slabs and is written
            // directly (no person-major copy, no transpose pass)
            float* ghpreT = slabs_f + (((int64_t)n_prf * lenf + 3) & ~(int64_t)3);
            hipLaunchKernelGGL(k_norm_enc_bwd_t64, dim3(nblk), dim3(256), 0, st, nb, W21, W22, h, gloc, graw, ghpreT, slabs_h);
            VX_CHECK_LAUNCH();
            if (seams().fc1_16) {
                ProfScope ps("k_fc1_bwd_c", st);                          // operands through LDS (k_fc1_bwd_c.hip), three bf16 terms
                rc = set_lds(k_fc1_bwd_c<false>, f1c_lds_bytes());             // (tmajor: nb % 4 == 0, ghpreT 16-byte aligned)
                if (rc) return rc;
                hipLaunchKernelGGL(k_fc1_bwd_c<false>, dim3((unsigned)((cfg->J + 1 + 511) / 512), (unsigned)n_prf), dim3(F1C_THREADS),
                                   f1c_lds_bytes(), st, dm, yT, yT_stride, ghpreT, slabs_f, lenf, (const uint32_t*)nullptr);
            } else {
                const size_t ldst = f1_lds_bytes(cfg->J);
                rc = set_lds(k_fc1_bwd_t, ldst);
                if (rc) return rc;
                hipLaunchKernelGGL(k_fc1_bwd_t, dim3((unsigned)((cfg->J + 511) / 512), (unsigned)n_prf), dim3(F1_THREADS), ldst, st,
                                   dm, yT, yT_stride, ghpreT, slabs_f, lenf);
            }
            VX_CHECK_LAUNCH();
            rc = vx_reduce_slabs(slabs_f, n_prf, lenf, -1.0f, genc, hs);
            if (rc) return rc;
            return vx_reduce_slabs(slabs_h, nblk, lenh, -1.0f, genc + lenf, hs);
        }
        hipLaunchKernelGGL(k_norm_enc_bwd_small, dim3(nblk), dim3(256), 2 * 256 * sizeof(float), st, (int)H, nb, W21, W22,
                           h, gloc, graw, ghpre, slabs_h);
        VX_CHECK_LAUNCH();
        // (a small batch: 128 items a workgroup, the form the multivariate guide's small batches take above)
        rc = fc1_bwd_person_major(dm, fc1_small_batch(dm.Hp, n_jg, n_prf), n_jg, n_prf, y, rows, ghpre, slabs_f, lenf, f1fast_ok(cfg, ghpre, y), st);
        if (rc) return rc;
    }
    rc = vx_reduce_slabs(slabs_f, n_prf, lenf, -1.0f, genc, hs);
    if (rc) return rc;
    return vx_reduce_slabs(slabs_h, nblk, lenh, -1.0f, genc + lenf, hs);
}

// ------------------------------------------------------------------------------------------------
// per wave a [C] table of 64-bit fixed-point sums (also used as a float table); the block reduce needs [waves][len] floats
static size_t hodina_lds_bytes(int C, int len) {
    const size_t tab = (size_t)HD_WAVES * C * sizeof(long long), red = (size_t)HD_WAVES * len * sizeof(float);
    return tab > red ? tab : red;
}
static int hodina_gsz(int64_t nb) { return hd_group_size(nb, (int64_t)num_cu() * 4 * HD_WAVES); }
static int hodina_blocks(int64_t nb) {
    const int64_t g = hodina_gsz(nb), n_groups = (nb + g - 1) / g;
    int64_t blocks = (n_groups + HD_WAVES - 1) / HD_WAVES;
    const int64_t cap = (int64_t)num_cu() * 4;
    if (blocks > cap) blocks = cap;
    return (int)(blocks < 1 ? 1 : blocks);
}

int64_t vx_hodina_workspace_floats(const vx_hodina_cfg* cfg, int64_t nb) {
    if (!hodina_cfg_ok(cfg) || nb < 0) return VX_EINVAL;
    return (int64_t)hodina_blocks(nb) * (2 * cfg->J + 2 * cfg->K);
}

int vx_hodina_grad(const vx_hodina_cfg* cfg, const uint8_t* y, const int64_t* rows, int64_t nb, int64_t gid0,
                   const float* loc, const float* raw, const float* eps_in, const float* q, const float* lam0,
                   const float* lam1_un, const float* g_un, const float* s_un, float* gloc, float* graw,
                   float* elbo, float* gitem, float* workspace, void* hs) {
    if (!hodina_cfg_ok(cfg) || !y || !loc || !raw || !q || !lam0 || !lam1_un || !g_un || !s_un || !gloc || !graw ||
        !elbo || !gitem || !workspace || nb < 0)
        return VX_EINVAL;
    const int blocks = hodina_blocks(nb);
    HoDinaDims dm;
    dm.K = cfg->K; dm.J = cfg->J; dm.C = 1 << cfg->K; dm.scale = cfg->scale; dm.nb = nb;
    dm.uniform_prior = 0; dm.dino = 0; dm.unmasked = 0;
    dm.step_dev = cfg->step_dev;
    dm.gsz = hodina_gsz(nb);
    const int len = 2 * cfg->J + 2 * cfg->K;
    hipStream_t st = (hipStream_t)hs;
    if (cfg->K >= 5 && cfg->K <= 8 && cfg->J <= 32) {
        // the pattern contractions on the bf16 MFMA, 32 persons per wave (k_hodina_m.hip); same slab layout
        const int NT = dm.C / 32;
        const size_t ldsm = hm_lds_bytes(NT);
        const int blocks_m = blocks < 2 * num_cu() ? blocks : 2 * num_cu();   // persistent (two blocks a CU): the operand images are built per block
        int rc = VX_EINVAL;
#define LAUNCH_HM(N)                                                                                          \
    rc = set_lds(k_hodina_m<N>, ldsm);                                                                        \
    if (rc) return rc;                                                                                        \
    hipLaunchKernelGGL((k_hodina_m<N>), dim3(blocks_m), dim3(HM_THREADS), ldsm, st, dm, y, rows, gid0, loc, raw, eps_in, \
                       cfg->seed, cfg->step, cfg->stream, q, lam0, lam1_un, g_un, s_un, gloc, graw, elbo, workspace)
        if (NT == 1) { LAUNCH_HM(1); } else if (NT == 2) { LAUNCH_HM(2); } else if (NT == 4) { LAUNCH_HM(4); } else { LAUNCH_HM(8); }
#undef LAUNCH_HM
        VX_CHECK_LAUNCH();
        return vx_reduce_slabs(workspace, blocks_m, len, -1.0f, gitem, hs);
    }
    const size_t lds = hodina_lds_bytes(dm.C, len);
    const int logcpl = cfg->K <= 8 ? 2 : (cfg->K == 9 ? 3 : 4);
    const int jpl = (cfg->J + 63) / 64;
#define LAUNCH_HD(L, JP)                                                                                      \
    hipLaunchKernelGGL((k_hodina<L, JP>), dim3(blocks), dim3(HD_THREADS), lds, st, dm, y, rows, gid0, loc, raw,   \
                       eps_in, cfg->seed, cfg->step, cfg->stream, q, lam0, lam1_un, g_un, s_un, gloc, graw, elbo, \
                       workspace)
#define DISPATCH_JPL(L)                              \
    if (jpl <= 1) { LAUNCH_HD(L, 1); }               \
    else if (jpl <= 2) { LAUNCH_HD(L, 2); }          \
    else if (jpl <= 4) { LAUNCH_HD(L, 4); }          \
    else if (jpl <= 8) { LAUNCH_HD(L, 8); }          \
    else { LAUNCH_HD(L, 16); }
    if (logcpl == 2) { DISPATCH_JPL(2) } else if (logcpl == 3) { DISPATCH_JPL(3) } else { DISPATCH_JPL(4) }
#undef DISPATCH_JPL
#undef LAUNCH_HD
    VX_CHECK_LAUNCH();
    return vx_reduce_slabs(workspace, blocks, len, -1.0f, gitem, hs);
}

// VCCDM (vi.py:819-865): the enumerated DINA / DINO with a uniform prior over the 2^K patterns -- the HO-DINA kernel
// without its theta / lambda side.  gitem = d LOSS / d [g_un: J | s_un: J]; elbo[nb] = per-person log marginal.
int64_t vx_ccdm_workspace_floats(const vx_hodina_cfg* cfg, int64_t nb) { return vx_hodina_workspace_floats(cfg, nb); }

int vx_ccdm_grad(const vx_hodina_cfg* cfg, int32_t dino, const uint8_t* y, const int64_t* rows, int64_t nb,
                 const float* q, const float* g_un, const float* s_un, float* elbo, float* gitem, float* workspace,
                 void* hs) {
    if (!hodina_cfg_ok(cfg) || !y || !q || !g_un || !s_un || !elbo || !gitem || !workspace || nb < 0) return VX_EINVAL;
    const int blocks = hodina_blocks(nb);
    HoDinaDims dm;
    dm.K = cfg->K; dm.J = cfg->J; dm.C = 1 << cfg->K; dm.scale = cfg->scale; dm.nb = nb;
    dm.uniform_prior = 1; dm.dino = dino ? 1 : 0; dm.unmasked = 0;
    dm.gsz = hodina_gsz(nb);
    const int len = 2 * cfg->J + 2 * cfg->K;                  // slab layout of k_hodina; the lambda tail stays zero
    const size_t lds = hodina_lds_bytes(dm.C, len);
    hipStream_t st = (hipStream_t)hs;
    const int logcpl = cfg->K <= 8 ? 2 : (cfg->K == 9 ? 3 : 4);
    const int jpl = (cfg->J + 63) / 64;
    const float* nul = nullptr;
    float* fnul = nullptr;
#define LAUNCH_CD(L, JP)                                                                                      \
    hipLaunchKernelGGL((k_hodina<L, JP>), dim3(blocks), dim3(HD_THREADS), lds, st, dm, y, rows, (int64_t)0, nul, nul, \
                       nul, (uint64_t)0, 0u, 0u, q, nul, nul, g_un, s_un, fnul, fnul, elbo, workspace)
#define DISPATCH_CD(L)                               \
    if (jpl <= 1) { LAUNCH_CD(L, 1); }               \
    else if (jpl <= 2) { LAUNCH_CD(L, 2); }          \
    else if (jpl <= 4) { LAUNCH_CD(L, 4); }          \
    else if (jpl <= 8) { LAUNCH_CD(L, 8); }          \
    else { LAUNCH_CD(L, 16); }
    if (logcpl == 2) { DISPATCH_CD(2) } else if (logcpl == 3) { DISPATCH_CD(3) } else { DISPATCH_CD(4) }
#undef DISPATCH_CD
#undef LAUNCH_CD
    VX_CHECK_LAUNCH();
    // the slabs carry [g | s | lam0 | lam1]: reduce the first 2 J entries of each
    hipLaunchKernelGGL(k_reduce_slabs, dim3(grid_1d(2 * cfg->J, 64)), dim3(256), 0, st, workspace, (int64_t)blocks,
                       (int64_t)len, (int64_t)(2 * cfg->J), -1.0f, gitem);
    VX_CHECK_LAUNCH();
    return VX_OK;
}


// ------------------------------------------------------------------------------------------------
// Person scores on a grid of latent nodes (k_grid_post.hip): two table builders and one kernel

// the persons of a call at the most, and the floats of a workspace it is handed
static const int64_t GRID_MAX_PERSONS = (int64_t)1 << 48;
// the shape limits of the entries that score against a node table (entries without persons pass nb = 1) ...
static bool grid_shape_ok(int64_t J, int64_t G, int64_t nb) {
    return J >= 1 && J <= GP_MAXJ && G >= 1 && G <= GP_MAXG && nb >= 1 && nb <= GRID_MAX_PERSONS;
}
// ... and of those that score at a point a person: vx_grid_pairs_*, vx_grid_fit_*, vx_grid_point_irt
static bool grid_point_shape_ok(int64_t J, int64_t nb) { return J >= 1 && J <= GP_MAXJ && nb >= 1 && nb <= GRID_MAX_PERSONS; }
// cells of the operand image, its zero padding included: what a table builder fills
static int64_t grid_image_cells(int J, int G) { return (int64_t)gp_nt(G) * 32 * gp_kc(J) * 16; }
// blocks of a person-on-lane launch (k_grid_post, k_grid_draw): a wave takes units of 32 * GP_MT persons, and the launch stops
// at two blocks a CU -- two waves a SIMD; a block's first act is to fill its LDS
static int grid_unit_blocks(int64_t nb) {
    const int64_t units = (nb + 32 * GP_MT - 1) / (32 * GP_MT);
    const int64_t blocks = (units + GP_WAVES - 1) / GP_WAVES, cap = (int64_t)num_cu() * 2;
    return (int)(blocks < cap ? blocks : cap);
}

int64_t vx_grid_image_bytes(int32_t J, int32_t G) {
    if (!grid_shape_ok(J, G, 1)) return VX_EINVAL;
    return gp_image_bytes(J, G);
}

int vx_grid_table_irt(const vx_irt_cfg* cfg, const float* theta, int32_t G, const float* a, const float* b, const float* c_un,
                      const float* d_un, void* img, void* hs) {
    if (!irt_items_ok(cfg, 4, GP_MAXD, a, b, c_un, d_un) || !grid_shape_ok(cfg->J, G, 1) || !theta || !img || !aligned16(img))
        return VX_EINVAL;
    const int blocks = grid_1d(grid_image_cells((int)cfg->J, (int)G), 256);
    return with_irt_model(cfg->model, [&](auto m) -> int {
        hipLaunchKernelGGL((k_grid_table_irt<decltype(m)::value>), dim3(blocks), dim3(256), 0, (hipStream_t)hs, (int)cfg->D, (int)cfg->J,
                           (int)G, cfg->Dc, theta, a, b, c_un, d_un, (uint16_t*)img);
        VX_CHECK_LAUNCH();
        return VX_OK;
    });
}

int vx_grid_table_cdm(const vx_hodina_cfg* cfg, int32_t dino, const float* q, const float* g_un, const float* s_un, void* img,
                      void* hs) {
    if (!cdm_items_ok(cfg, dino, q, g_un, s_un) || !img || !aligned16(img)) return VX_EINVAL;
    hipLaunchKernelGGL(k_grid_table_cdm, dim3(grid_1d(grid_image_cells((int)cfg->J, 1 << cfg->K), 256)), dim3(256), 0, (hipStream_t)hs,
                       (int)cfg->K, (int)cfg->J, (int)dino, q, g_un, s_un, (uint16_t*)img);
    VX_CHECK_LAUNCH();
    return VX_OK;
}

int vx_grid_posterior(const uint8_t* y, const int64_t* rows, int64_t nb, int32_t J, int32_t G, int32_t D, const void* img,
                      const float* logw, const float* coord, float* loglik, float* mean, float* sd, int32_t* argmax, void* hs) {
    if (!y || !img || !aligned16(img) || !logw || !coord || !loglik || !mean || !sd || !argmax) return VX_EINVAL;
    if (!grid_shape_ok(J, G, nb) || D < 1 || D > GP_MAXD) return VX_EINVAL;
    const int blocks = grid_unit_blocks(nb);
    hipStream_t st = (hipStream_t)hs;
    const uint4* im = (const uint4*)img;
#define LAUNCH_GP(DPV)                                                                                                \
    hipLaunchKernelGGL((k_grid_post<DPV>), dim3(blocks), dim3(GP_THREADS), (size_t)gp_nt(G) * 32 * (DPV + 1) * sizeof(float), \
                       st, y, rows, nb, (int)J, (int)G, (int)D, im, logw, coord, loglik, mean, sd, argmax)
    if (D == 1) { LAUNCH_GP(1); } else if (D == 2) { LAUNCH_GP(2); } else if (D == 3) { LAUNCH_GP(3); }
    else if (D == 4) { LAUNCH_GP(4); } else if (D <= 6) { LAUNCH_GP(6); } else if (D <= 8) { LAUNCH_GP(8); } else { LAUNCH_GP(10); }
#undef LAUNCH_GP
    VX_CHECK_LAUNCH();
    return VX_OK;
}

// Bifactor / testlet scores (k_grid_bifactor.hip): the table builder, the kernel of the general marginal, the specific moments.
// tl_start is HOST memory (checked here; tl_start_dev is the same table on the device, which the kernels read).
int64_t vx_grid_bifactor_image_bytes(int32_t Gg, int32_t KC) {
    if (!gb_shape_ok(Gg, 1, KC, 1, 1, GRID_MAX_PERSONS)) return VX_EINVAL;
    return gb_image_bytes(Gg, KC);
}

int64_t vx_grid_bifactor_workspace_floats(int64_t nb, int32_t Gg) {
    if (!gb_shape_ok(Gg, 1, 1, 1, nb, GRID_MAX_PERSONS)) return VX_EINVAL;
    return gb_ws_floats(nb, Gg);
}

int vx_grid_table_bifactor(const vx_irt_cfg* cfg, const float* theta_g, int32_t Gg, const float* u, int32_t Gh, int32_t general,
                           const int32_t* col, const int32_t* sdim, int32_t KC, const float* a, const float* b, const float* c_un,
                           const float* d_un, void* img, void* hs) {
    if (!irt_items_ok(cfg, 4, GB_MAXD, a, b, c_un, d_un) || cfg->model < 2 || cfg->D < 2 || cfg->J < 1 || cfg->J > GP_MAXJ)
        return VX_EINVAL;
    if (!gb_shape_ok(Gg, Gh, KC, 1, 1, GRID_MAX_PERSONS) || general < 0 || general >= cfg->D) return VX_EINVAL;
    if (!theta_g || !u || !col || !sdim || !img || !aligned16(img)) return VX_EINVAL;
    const int blocks = grid_1d((int64_t)Gg * 32 * KC * 16, 256);
    return with_irt_model(cfg->model, [&](auto m) -> int {
        hipLaunchKernelGGL((k_grid_table_bifactor<decltype(m)::value>), dim3(blocks), dim3(256), 0, (hipStream_t)hs, (int)cfg->D,
                           (int)cfg->J, (int)Gg, (int)Gh, (int)KC, (int)general, cfg->Dc, theta_g, u, col, sdim, a, b, c_un, d_un,
                           (uint16_t*)img);
        VX_CHECK_LAUNCH();
        return VX_OK;
    });
}

int vx_grid_bifactor(const uint8_t* y, int64_t nb, int32_t KC, int32_t Gg, int32_t Gh, const int32_t* tl_start, int32_t n_tl,
                     const int32_t* tl_start_dev, const void* img, const float* logw, const float* coord, const float* logv,
                     const float* u, float* loglik, float* mean, float* sd, int32_t* argmax, float* fws, void* hs) {
    if (!y || !tl_start_dev || !img || !aligned16(img) || !logw || !coord || !logv || !u || !loglik || !mean || !sd || !argmax)
        return VX_EINVAL;
    if (!gb_shape_ok(Gg, Gh, KC, n_tl, nb, GRID_MAX_PERSONS) || !gb_testlets_ok(tl_start, (int)n_tl, (int)KC)) return VX_EINVAL;
    hipLaunchKernelGGL(k_grid_bifactor, dim3(grid_unit_blocks(nb)), dim3(GP_THREADS), 0, (hipStream_t)hs, y, nb, (int)KC, (int)Gg,
                       (int)Gh, tl_start_dev, (int)n_tl, (const uint4*)img, logw, coord, logv, u, loglik, mean, sd, argmax, fws);
    VX_CHECK_LAUNCH();
    return VX_OK;
}

int vx_grid_bifactor_specific(const uint8_t* y, int64_t nb, int32_t KC, int32_t Gg, int32_t Gh, const int32_t* tl_start,
                              int32_t n_tl, const int32_t* tl_start_dev, const void* img, const float* logv, const float* u,
                              const float* loglik, const float* fws, float* mean_s, float* sd_s, void* hs) {
    if (!y || !tl_start_dev || !img || !aligned16(img) || !logv || !u || !loglik || !fws || !mean_s || !sd_s) return VX_EINVAL;
    if (!gb_shape_ok(Gg, Gh, KC, n_tl, nb, GRID_MAX_PERSONS) || !gb_testlets_ok(tl_start, (int)n_tl, (int)KC)) return VX_EINVAL;
    hipLaunchKernelGGL(k_grid_bifactor_spec, dim3(grid_unit_blocks(nb)), dim3(GP_THREADS), 0, (hipStream_t)hs, y, nb, (int)KC,
                       (int)Gg, (int)Gh, tl_start_dev, (int)n_tl, (const uint4*)img, logv, u, loglik, fws, mean_s, sd_s);
    VX_CHECK_LAUNCH();
    return VX_OK;
}

// Expected counts of a bifactor model (k_grid_bifactor_counts.hip): one kernel over (chunk groups x node pairs x person chunks),
// then the chunks' slabs added in ascending order and scattered to the model's item order
int64_t vx_grid_bifactor_counts_workspace_floats(int64_t nb, int32_t KC, int32_t Gg, int32_t n_tl) {
    if (!gb_shape_ok(Gg, 1, KC, n_tl, nb, GRID_MAX_PERSONS)) return VX_EINVAL;
    const GbcPlan p = gbc_plan(nb, (int)KC, (int)Gg, (int)n_tl);
    return p.n_chunks * p.slab_len;
}

int vx_grid_bifactor_counts(const uint8_t* y, int64_t nb, int32_t KC, int32_t Gg, int32_t Gh, const int32_t* tl_start, int32_t n_tl,
                            const int32_t* tl_start_dev, const int32_t* col, int32_t J, const void* img, const float* logv,
                            const float* loglik, const float* fws, int32_t accumulate, float* n1, float* n0, float* mass,
                            float* mass_s, float* workspace, void* hs) {
    if (!y || !tl_start_dev || !col || !img || !aligned16(img) || !logv || !loglik || !fws || !n1 || !n0 || !mass || !workspace ||
        !aligned16(workspace))
        return VX_EINVAL;
    if (J < 1 || J > GP_MAXJ || (accumulate != 0 && accumulate != 1)) return VX_EINVAL;
    if (!gb_shape_ok(Gg, Gh, KC, n_tl, nb, GRID_MAX_PERSONS) || !gb_testlets_ok(tl_start, (int)n_tl, (int)KC)) return VX_EINVAL;
    const GbcPlan p = gbc_plan(nb, (int)KC, (int)Gg, (int)n_tl);
    const int n_groups = gbc_groups(tl_start, (int)n_tl);
    hipStream_t st = (hipStream_t)hs;
    hipLaunchKernelGGL(k_grid_bifactor_counts, dim3((unsigned)n_groups, (unsigned)p.n_gpairs, (unsigned)p.n_chunks), dim3(GP_THREADS), 0,
                       st, y, nb, (int)KC, (int)Gg, (int)Gh, tl_start_dev, (int)n_tl, (const uint4*)img, logv, loglik, fws,
                       p.units_per_chunk, workspace, p.slab_len);
    VX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_grid_bifactor_counts_reduce, dim3(grid_1d(p.slab_len, 256)), dim3(256), 0, st, workspace, p.n_chunks,
                       p.slab_len, (int)KC, (int)Gg, (int)Gh, (int)n_tl, col, (int)J, (int)accumulate, n1, n0, mass, mass_s);
    VX_CHECK_LAUNCH();
    return VX_OK;
}

// Plausible values (k_grid_draw.hip): the draws go to launches of PV_CAP slots that start at multiples of 4, so that a Philox
// call (four draws) never straddles two launches; what a draw is does not depend on the cut
int vx_grid_draw(const uint8_t* y, const int64_t* rows, int64_t nb, int32_t J, int32_t G, const void* img, const float* logw,
                 uint64_t seed, int64_t row_offset, int32_t draw0, int32_t ndraws, int64_t stride, int32_t* node, void* hs) {
    if (!y || !img || !aligned16(img) || !logw || !node) return VX_EINVAL;
    if (!grid_shape_ok(J, G, nb) || !draw_range_ok(draw0, ndraws, stride)) return VX_EINVAL;
    const int blocks = grid_unit_blocks(nb);
    const int hi = draw0 + ndraws;
    for (int base = draw0 & ~3; base < hi; base += PV_CAP) {
        hipLaunchKernelGGL(k_grid_draw, dim3(blocks), dim3(GP_THREADS), pv_lds_bytes(G), (hipStream_t)hs, y, rows, nb, (int)J,
                           (int)G, (const uint4*)img, logw, seed, row_offset, base, (int)draw0, hi, stride, node);
        VX_CHECK_LAUNCH();
    }
    return VX_OK;
}

// The conditioned entries (k_grid_cond.hip): vx_grid_posterior / vx_grid_draw with a tilt a person; launch shapes as theirs
int vx_grid_posterior_cond(const uint8_t* y, const int64_t* rows, int64_t nb, int32_t J, int32_t G, int32_t D, const void* img,
                           const float* logw, const float* coord, const float* tilt, float* logjoint, float* lognorm, float* mean,
                           float* cov, int32_t* argmax, void* hs) {
    if (!y || !img || !aligned16(img) || !logw || !coord || !tilt || !logjoint || !lognorm || !mean || !cov || !argmax) return VX_EINVAL;
    if (!grid_shape_ok(J, G, nb) || D < 1 || D > GPC_MAXD) return VX_EINVAL;
    const int blocks = grid_unit_blocks(nb);
    hipStream_t st = (hipStream_t)hs;
    const uint4* im = (const uint4*)img;
#define LAUNCH_GPC(DPV)                                                                                               \
    hipLaunchKernelGGL((k_grid_post_cond<DPV>), dim3(blocks), dim3(GP_THREADS), (size_t)gp_nt(G) * 32 * (DPV + 1) * sizeof(float), \
                       st, y, rows, nb, (int)J, (int)G, (int)D, im, logw, coord, tilt, logjoint, lognorm, mean, cov, argmax)
    if (D == 1) { LAUNCH_GPC(1); } else if (D == 2) { LAUNCH_GPC(2); } else { LAUNCH_GPC(3); }
#undef LAUNCH_GPC
    VX_CHECK_LAUNCH();
    return VX_OK;
}

int vx_grid_draw_cond(const uint8_t* y, const int64_t* rows, int64_t nb, int32_t J, int32_t G, int32_t D, const void* img,
                      const float* logw, const float* coord, const float* tilt, uint64_t seed, int64_t row_offset, int32_t draw0,
                      int32_t ndraws, int64_t stride, int32_t* node, void* hs) {
    if (!y || !img || !aligned16(img) || !logw || !coord || !tilt || !node) return VX_EINVAL;
    if (!grid_shape_ok(J, G, nb) || D < 1 || D > GPC_MAXD || !draw_range_ok(draw0, ndraws, stride)) return VX_EINVAL;
    const int blocks = grid_unit_blocks(nb);
    const int hi = draw0 + ndraws;
    for (int base = draw0 & ~3; base < hi; base += PVC_CAP) {
        hipLaunchKernelGGL(k_grid_draw_cond, dim3(blocks), dim3(GP_THREADS), pvc_lds_bytes(G), (hipStream_t)hs, y, rows, nb, (int)J,
                           (int)G, (int)D, (const uint4*)img, logw, coord, tilt, seed, row_offset, base, (int)draw0, hi, stride,
                           node);
        VX_CHECK_LAUNCH();
    }
    return VX_OK;
}

// Expected counts from the grid posteriors (k_grid_counts.hip): one kernel over (node groups x person chunks), then the chunks'
// slabs added in ascending order
int64_t vx_grid_counts_workspace_floats(int64_t nb, int32_t J, int32_t G) {
    if (!grid_shape_ok(J, G, nb)) return VX_EINVAL;
    const GcPlan p = gc_plan(nb, J, G);
    return p.n_chunks * p.slab_len;
}

int vx_grid_counts(const uint8_t* y, const int64_t* rows, int64_t nb, int32_t J, int32_t G, const void* img, const float* logw,
                   const float* loglik, float* n1, float* n0, float* mass, float* workspace, void* hs) {
    if (!y || !img || !aligned16(img) || !logw || !loglik || !n1 || !n0 || !mass || !workspace) return VX_EINVAL;
    if (!grid_shape_ok(J, G, nb)) return VX_EINVAL;
    const GcPlan p = gc_plan(nb, J, G);
    hipStream_t st = (hipStream_t)hs;
    const int rc = with_counts_tiles(p.it, [&](auto it, auto ntg) -> int {
        constexpr int IT = decltype(it)::value, NTG = decltype(ntg)::value;
        return launch_lds(k_grid_counts<IT, NTG>, dim3((unsigned)(p.n_groups * p.n_chunks)), dim3(GC_THREADS), gc_lds_bytes<NTG>(), st,
                          y, rows, nb, (int)J, (int)G, (const uint4*)img, logw, loglik, p.n_groups, p.rounds_per_chunk, workspace,
                          p.slab_len);
    });
    if (rc) return rc;
    return counts_reduce(J, G, n1, n0, mass, [&](int64_t off, int64_t len, float* out) {
        hipLaunchKernelGGL(k_reduce_slabs, dim3(grid_1d(len, 64)), dim3(256), 0, st, workspace + off, p.n_chunks, p.slab_len, len, 1.0f,
                           out);
    });
}

// Expected counts under a tilt a person, a table set a segment (k_grid_counts_cond.hip): the plan's table into the head of the
// workspace (from kernel arguments), one kernel over (the chunks of all segments x node groups), then every segment's slabs added
// in ascending order.  seg_start is HOST memory: it is checked and planned from here, and not used after the call returns.
int64_t vx_grid_counts_cond_workspace_floats(int64_t nb, int32_t n_seg, int32_t J, int32_t G) {
    if (!grid_shape_ok(J, G, nb) || n_seg < 1 || n_seg > GCC_MAXSEG) return VX_EINVAL;
    const GccPlan p = gcc_plan(nb, n_seg, J, G);
    return p.tab_floats + p.max_chunks * p.gc.slab_len;
}

int vx_grid_counts_cond(const uint8_t* y, const int64_t* rows, int64_t nb, int32_t J, int32_t G, int32_t D, const void* img,
                        const float* logw, const float* coord, const float* tilt, const float* logjoint, const int64_t* seg_start,
                        int32_t n_seg, float* n1, float* n0, float* mass, float* workspace, void* hs) {
    if (!y || !img || !aligned16(img) || !logw || !coord || !tilt || !logjoint || !seg_start || !n1 || !n0 || !mass || !workspace ||
        !aligned16(workspace))
        return VX_EINVAL;
    if (!grid_shape_ok(J, G, nb) || D < 1 || D > GPC_MAXD || n_seg < 1 || n_seg > GCC_MAXSEG) return VX_EINVAL;
    if (seg_start[0] != 0 || seg_start[n_seg] != nb) return VX_EINVAL;
    for (int s = 0; s < n_seg; ++s)
        if (seg_start[s + 1] < seg_start[s]) return VX_EINVAL;
    const GccPlan p = gcc_plan(nb, n_seg, J, G);
    // the table: [seg_start (n_seg + 1) | chunk_start (n_seg + 1)]
    std::vector<int64_t> tab(2 * ((size_t)n_seg + 1));
    const int64_t rpc = gcc_rounds_per_chunk(seg_start, (int)n_seg, p.gc);
    int64_t chunks = 0;
    for (int s = 0; s <= n_seg; ++s) {
        tab[s] = seg_start[s];
        tab[(size_t)n_seg + 1 + s] = chunks;
        if (s < n_seg) chunks += gcc_chunks(seg_start[s + 1] - seg_start[s], rpc);
    }
    if (chunks < 1 || chunks > p.max_chunks) return VX_EINVAL;                      // (cannot happen: gcc_plan's bound)
    hipStream_t st = (hipStream_t)hs;
    int64_t* dtab = (int64_t*)workspace;
    for (size_t o = 0; o < tab.size(); o += GCC_TAB_VALUES) {
        GccTabArgs a;
        const int n = (int)(tab.size() - o < GCC_TAB_VALUES ? tab.size() - o : GCC_TAB_VALUES);
        for (int i = 0; i < GCC_TAB_VALUES; ++i) a.v[i] = i < n ? tab[o + i] : 0;
        hipLaunchKernelGGL(k_gcc_table, dim3(1), dim3(GCC_TAB_VALUES), 0, st, a, n, dtab + o);
        VX_CHECK_LAUNCH();
    }
    float* slabs = workspace + p.tab_floats;
    const int rc = with_counts_tiles(p.gc.it, [&](auto it, auto ntg) -> int {
        constexpr int IT = decltype(it)::value, NTG = decltype(ntg)::value;
        return launch_lds(k_grid_counts_cond<IT, NTG>, dim3((unsigned)(p.gc.n_groups * chunks)), dim3(GC_THREADS), gcc_lds_bytes<NTG>(),
                          st, y, rows, (int)J, (int)G, (int)D, (const uint4*)img, logw, coord, tilt, logjoint, (const int64_t*)dtab,
                          (int)n_seg, p.gc.n_groups, slabs, p.gc.slab_len);
    });
    if (rc) return rc;
    return counts_reduce(J, G, n1, n0, mass, [&](int64_t off, int64_t len, float* out) {
        hipLaunchKernelGGL(k_reduce_segments, dim3(grid_1d(len, 64), (unsigned)n_seg), dim3(256), 0, st, slabs + off, (const int64_t*)dtab,
                           (int)n_seg, p.gc.slab_len, len, out);
    });
}

// The M-step on the expected-count tables (k_grid_mstep.hip): one wave an item, every Newton step inside the one launch.  One
// launcher behind both entries; `penalised` is the kernel's PRIOR: all four models, with a normal prior an unknown.
static int grid_mstep_irt(bool penalised, const vx_irt_cfg* cfg, const float* theta, int32_t G, const float* n1, const float* n0,
                          const float* a_free, float* a, float* b, float* c_un, float* d_un, const float* prior, int32_t newton,
                          float* lprior, void* hs) {
    if (!irt_items_ok(cfg, penalised ? 4 : 2, GM_MAXD, a, b, c_un, d_un) || !grid_shape_ok(cfg->J, G, 1) || newton < 1 ||
        newton > GM_MAX_NEWTON || !theta || !n1 || !n0 || (penalised && !prior))
        return VX_EINVAL;
    const dim3 grid((unsigned)((cfg->J + GM_WAVES - 1) / GM_WAVES));
    return with_irt_model(cfg->model, [&](auto m) -> int {
        auto launch = [&](auto pr) -> int {
            constexpr bool PRIOR = decltype(pr)::value;
            constexpr int M = PRIOR || decltype(m)::value < 2 ? decltype(m)::value : 2;     // (without a prior the gate admits 1PL and 2PL only)
            hipLaunchKernelGGL((k_grid_mstep_irt<M, PRIOR>), grid, dim3(GM_THREADS), 0, (hipStream_t)hs, (int)cfg->D, (int)cfg->J, (int)G,
                               cfg->Dc, theta, n1, n0, a_free, a, b, c_un, d_un, prior, lprior, (int)newton);
            VX_CHECK_LAUNCH();
            return VX_OK;
        };
        return penalised ? launch(std::true_type()) : launch(std::false_type());
    });
}

int vx_grid_mstep_irt(const vx_irt_cfg* cfg, const float* theta, int32_t G, const float* n1, const float* n0, const float* a_free,
                      float* a, float* b, int32_t newton, void* hs) {
    return grid_mstep_irt(false, cfg, theta, G, n1, n0, a_free, a, b, nullptr, nullptr, nullptr, newton, nullptr, hs);
}

// The precisions live in device memory: that they are >= 0 and finite is checked where `prior` is made (vipsy_amd/grid.py).
int vx_grid_mstep_irt_map(const vx_irt_cfg* cfg, const float* theta, int32_t G, const float* n1, const float* n0, const float* a_free,
                          float* a, float* b, float* c_un, float* d_un, const float* prior, int32_t newton, float* lprior, void* hs) {
    return grid_mstep_irt(true, cfg, theta, G, n1, n0, a_free, a, b, c_un, d_un, prior, newton, lprior, hs);
}

int vx_grid_mstep_cdm(const vx_hodina_cfg* cfg, int32_t dino, const float* q, const float* n1, const float* n0, float* g_un,
                      float* s_un, void* hs) {
    if (!cdm_items_ok(cfg, dino, q, g_un, s_un) || !n1 || !n0) return VX_EINVAL;
    hipLaunchKernelGGL(k_grid_mstep_cdm, dim3((unsigned)((cfg->J + GM_WAVES - 1) / GM_WAVES)), dim3(GM_THREADS), 0, (hipStream_t)hs,
                       (int)cfg->K, (int)cfg->J, (int)dino, q, n1, n0, g_un, s_un);
    VX_CHECK_LAUNCH();
    return VX_OK;
}

// Item-parameter information from the grid posteriors (k_grid_info.hip): derivative tables, person scores, the SYRK over persons
static bool grid_info_shape_ok(int64_t J, int64_t G, int64_t K, int64_t nb) {
    return grid_shape_ok(J, G, nb) && K >= 1 && K <= GI_MAXK && J * K <= GI_MAXP;
}
static bool grid_wimage_shape_ok(int64_t P, int64_t G) { return P >= 1 && P <= GI_MAXP && G >= 1 && G <= GP_MAXG; }

int64_t vx_grid_wimage_bytes(int32_t P, int32_t G) {
    if (!grid_wimage_shape_ok(P, G)) return VX_EINVAL;
    return gi_wimage_frag_bytes(P, G) + 16;
}

int vx_grid_wtable_irt(const vx_irt_cfg* cfg, const float* theta, int32_t G, const float* a, const float* b, void* wimg, void* hs) {
    if (!irt_items_ok(cfg, 2, GM_MAXD, a, b, nullptr, nullptr) || !grid_shape_ok(cfg->J, G, 1) || !theta || !wimg || !aligned16(wimg))
        return VX_EINVAL;
    const int P = (int)cfg->J * (cfg->model == 1 ? 1 : (int)cfg->D + 1);
    const int blocks = grid_1d((int64_t)gp_nt(G) * 32 * gi_pt(P) * 32, 256);
    float* trailer = (float*)((uint8_t*)wimg + gi_wimage_frag_bytes(P, G));
    return with_irt_model(cfg->model, [&](auto m) -> int {
        constexpr int M = decltype(m)::value < 2 ? 1 : 2;                               // (the gate admits 1PL and 2PL only)
        hipLaunchKernelGGL((k_grid_wtable_irt<M>), dim3(blocks), dim3(256), 0, (hipStream_t)hs, (int)cfg->D, (int)cfg->J, (int)G, cfg->Dc,
                           theta, a, b, (uint16_t*)wimg, trailer);
        VX_CHECK_LAUNCH();
        return VX_OK;
    });
}

// The tables at the fit of vx_grid_mstep_irt_map: models 1 and 2 are vx_grid_wtable_irt's launch; 3 and 4 take the scale from the
// table itself (k_grid_wtable_irt_asym: the maximum, the trailer, the image)
int vx_grid_wtable_irt_map(const vx_irt_cfg* cfg, const float* theta, int32_t G, const float* a, const float* b, const float* c_un,
                           const float* d_un, void* wimg, void* hs) {
    if (!irt_items_ok(cfg, 4, GM_MAXD, a, b, c_un, d_un) || !grid_shape_ok(cfg->J, G, 1) || !theta || !wimg || !aligned16(wimg))
        return VX_EINVAL;
    if (cfg->model <= 2) return vx_grid_wtable_irt(cfg, theta, G, a, b, wimg, hs);
    const int64_t P64 = (int64_t)cfg->J * (cfg->D + cfg->model - 1);
    if (P64 > GI_MAXP) return VX_EINVAL;
    const int P = (int)P64;
    const int blocks = grid_1d((int64_t)gp_nt(G) * 32 * gi_pt(P) * 32, 256);
    hipStream_t st = (hipStream_t)hs;
    float* trailer = (float*)((uint8_t*)wimg + gi_wimage_frag_bytes(P, G));
    if (hipError_t he = hipMemsetAsync(trailer, 0, 16, st)) return (int)he;
    return with_irt_model(cfg->model, [&](auto m) -> int {
        constexpr int M = decltype(m)::value < 4 ? 3 : 4;                               // (models 1 and 2 have left above)
        hipLaunchKernelGGL((k_grid_wtable_irt_asym<M, false>), dim3(blocks), dim3(256), 0, st, (int)cfg->D, (int)cfg->J, (int)G, cfg->Dc,
                           theta, a, b, c_un, d_un, (uint16_t*)wimg, trailer);
        VX_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_grid_wscale, dim3(1), dim3(1), 0, st, trailer);
        VX_CHECK_LAUNCH();
        hipLaunchKernelGGL((k_grid_wtable_irt_asym<M, true>), dim3(blocks), dim3(256), 0, st, (int)cfg->D, (int)cfg->J, (int)G, cfg->Dc,
                           theta, a, b, c_un, d_un, (uint16_t*)wimg, trailer);
        VX_CHECK_LAUNCH();
        return VX_OK;
    });
}

int vx_grid_wtable_cdm(const vx_hodina_cfg* cfg, int32_t dino, const float* q, const float* g_un, const float* s_un, void* wimg,
                       void* hs) {
    if (!cdm_items_ok(cfg, dino, q, g_un, s_un) || !wimg || !aligned16(wimg)) return VX_EINVAL;
    const int P = 2 * (int)cfg->J, G = 1 << cfg->K;
    float* trailer = (float*)((uint8_t*)wimg + gi_wimage_frag_bytes(P, G));
    hipLaunchKernelGGL(k_grid_wtable_cdm, dim3(grid_1d((int64_t)gp_nt(G) * 32 * gi_pt(P) * 32, 256)), dim3(256), 0, (hipStream_t)hs,
                       (int)cfg->K, (int)cfg->J, (int)dino, q, g_un, s_un, (uint16_t*)wimg, trailer);
    VX_CHECK_LAUNCH();
    return VX_OK;
}

int64_t vx_grid_info_workspace_floats(int64_t nb, int32_t P, int32_t G) {
    if (!grid_wimage_shape_ok(P, G) || nb < 1 || nb > GRID_MAX_PERSONS) return VX_EINVAL;
    return gi_slab_plan(nb, P, -1).total;
}

int64_t vx_grid_info_workspace_min_floats(int32_t P, int32_t G) {
    if (!grid_wimage_shape_ok(P, G)) return VX_EINVAL;
    return gi_slab_min_floats(P);
}

int vx_grid_info(const uint8_t* y, const int64_t* rows, int64_t nb, int32_t J, int32_t G, int32_t K, const void* img, const void* wimg,
                 const float* logw, const float* loglik, float* info, float* gradient, float* workspace, int64_t ws_floats, void* hs) {
    if (!y || !img || !aligned16(img) || !wimg || !aligned16(wimg) || !logw || !loglik || !info || !gradient || !workspace ||
        !aligned16(workspace))
        return VX_EINVAL;
    if (!grid_info_shape_ok(J, G, K, nb)) return VX_EINVAL;
    const int P = (int)J * (int)K;
    if (ws_floats < gi_slab_min_floats(P) || ws_floats > GRID_MAX_PERSONS) return VX_EINVAL;
    const SlabPlan p = gi_slab_plan(nb, P, ws_floats);
    hipStream_t st = (hipStream_t)hs;
    const float* trailer = (const float*)((const uint8_t*)wimg + gi_wimage_frag_bytes(P, G));
    const size_t lds = gi_lds_bytes(G);
    const int rc = set_lds(k_grid_pscores, lds);
    if (rc) return rc;
    // k_grid_pscores writes whole units of 64 persons: GP_MT units of 32 each
    auto frag = [&](int64_t i0, int64_t ns) -> int64_t {
        const int64_t units64 = (ns + 32 * GP_MT - 1) / (32 * GP_MT), cap = (int64_t)num_cu() * 2;
        hipLaunchKernelGGL(k_grid_pscores, dim3((unsigned)(units64 < cap ? units64 : cap)), dim3(GP_THREADS), lds, st,
                           rows ? y : y + i0 * J, rows ? rows + i0 : rows, ns, (int)J, (int)G, (int)K, P, (const uint4*)img,
                           (const uint4*)wimg, trailer, logw, loglik + i0, (uint4*)workspace, gi_nsub(G));
        return units64 * GP_MT;
    };
    return grid_slab_loop(p, nb, workspace, hs, k_grid_xprod, 256, frag, [&] {
        hipLaunchKernelGGL(k_info_finish, dim3(grid_1d((int64_t)P * (P + 1), 256)), dim3(256), 0, st,
                           (const float*)(workspace + p.off_acc), P, p.tiles, trailer, info, gradient);
    });
}

// Local dependence (k_grid_pairs.hip): the residual cell as operand fragments, the masked cross products over persons, the sums
int64_t vx_grid_pairs_workspace_floats(int64_t nb, int32_t J) {
    if (!grid_point_shape_ok(J, nb)) return VX_EINVAL;
    return pp_slab_plan(nb, J, -1).total;
}

int64_t vx_grid_pairs_workspace_min_floats(int32_t J) {
    if (!grid_point_shape_ok(J, 1)) return VX_EINVAL;
    return pp_slab_min_floats(J);
}

int vx_grid_pairs_irt(const vx_irt_cfg* cfg, const uint8_t* y, const int64_t* rows, int64_t nb, const float* theta_hat, const float* a,
                      const float* b, const float* c_un, const float* d_un, float* n, float* s, float* ss, float* sp, float* workspace,
                      int64_t ws_floats, void* hs) {
    if (!irt_items_ok(cfg, 4, PP_MAXD, a, b, c_un, d_un) || !grid_point_shape_ok(cfg->J, nb)) return VX_EINVAL;
    if (!y || !theta_hat || !n || !s || !ss || !sp || !workspace || !aligned16(workspace)) return VX_EINVAL;
    if (ws_floats < pp_slab_min_floats((int)cfg->J) || ws_floats > GRID_MAX_PERSONS) return VX_EINVAL;
    hipStream_t st = (hipStream_t)hs;
    const int D = (int)cfg->D, J = (int)cfg->J;
    return grid_pairs_run(nb, J, n, s, ss, sp, workspace, ws_floats, hs, [&](int64_t i0, int64_t ns, int64_t n_units, dim3 grid) {
        with_irt_model(cfg->model, [&](auto m) -> int {
            hipLaunchKernelGGL((k_pair_frag<decltype(m)::value>), grid, dim3(256), 0, st, rows ? y : y + i0 * J, rows ? rows + i0 : rows, ns,
                               D, J, cfg->Dc, theta_hat + i0 * D, a, b, c_un, d_un, (uint4*)workspace, n_units);
            return VX_OK;
        });
    });
}

int vx_grid_pairs_cdm(const vx_hodina_cfg* cfg, int32_t dino, const float* q, const uint8_t* y, const int64_t* rows, int64_t nb,
                      const int32_t* pattern, const float* g_un, const float* s_un, float* n, float* s, float* ss, float* sp,
                      float* workspace, int64_t ws_floats, void* hs) {
    if (!cdm_items_ok(cfg, dino, q, g_un, s_un) || !grid_point_shape_ok(cfg->J, nb)) return VX_EINVAL;
    if (!y || !pattern || !n || !s || !ss || !sp || !workspace || !aligned16(workspace)) return VX_EINVAL;
    if (ws_floats < pp_slab_min_floats((int)cfg->J) || ws_floats > GRID_MAX_PERSONS) return VX_EINVAL;
    hipStream_t st = (hipStream_t)hs;
    const int K = (int)cfg->K, J = (int)cfg->J;
    return grid_pairs_run(nb, J, n, s, ss, sp, workspace, ws_floats, hs, [&](int64_t i0, int64_t ns, int64_t n_units, dim3 grid) {
        hipLaunchKernelGGL(k_pair_frag_cdm, grid, dim3(256), 0, st, rows ? y : y + i0 * J, rows ? rows + i0 : rows, ns, K, J, (int)dino, q,
                           pattern + i0, g_un, s_un, (uint4*)workspace, n_units);
    });
}

// Person fit (k_grid_fit.hip): the sums behind lz and infit / outfit per person and per item, one pass over persons x items
int64_t vx_grid_fit_workspace_floats(int64_t nb, int32_t J) {
    if (!grid_point_shape_ok(J, nb)) return VX_EINVAL;
    return gf_ws_floats(nb, J);
}

// the item partials of the workgroups, added in ascending order
static int grid_fit_finish(const GfPlan& p, int J, const float* workspace, float* item, void* hs) {
    VX_CHECK_LAUNCH();
    const int len = GF_ITEM * J;
    hipLaunchKernelGGL(k_fit_items, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, (hipStream_t)hs, workspace, p.n_blocks, len, item);
    VX_CHECK_LAUNCH();
    return VX_OK;
}

int vx_grid_fit_irt(const vx_irt_cfg* cfg, const uint8_t* y, const int64_t* rows, int64_t nb, const float* theta_hat, const float* a,
                    const float* b, const float* c_un, const float* d_un, float* person, float* item, float* workspace,
                    int64_t ws_floats, void* hs) {
    if (!irt_items_ok(cfg, 4, GF_MAXD, a, b, c_un, d_un) || !grid_point_shape_ok(cfg->J, nb)) return VX_EINVAL;
    if (!y || !theta_hat || !person || !item || !workspace) return VX_EINVAL;
    if (ws_floats < gf_ws_floats(nb, (int)cfg->J)) return VX_EINVAL;
    const int D = (int)cfg->D, J = (int)cfg->J;
    const GfPlan p = gf_plan(nb);
    with_irt_model(cfg->model, [&](auto m) -> int {
        hipLaunchKernelGGL((k_fit_irt<decltype(m)::value>), dim3((unsigned)p.n_blocks), dim3(256), 0, (hipStream_t)hs, y, rows, nb, D, J,
                           cfg->Dc, theta_hat, a, b, c_un, d_un, person, workspace, p.n_units, p.units_per_block);
        return VX_OK;
    });
    return grid_fit_finish(p, J, workspace, item, hs);
}

int vx_grid_fit_cdm(const vx_hodina_cfg* cfg, int32_t dino, const float* q, const uint8_t* y, const int64_t* rows, int64_t nb,
                    const int32_t* pattern, const float* g_un, const float* s_un, float* person, float* item, float* workspace,
                    int64_t ws_floats, void* hs) {
    if (!cdm_items_ok(cfg, dino, q, g_un, s_un) || !grid_point_shape_ok(cfg->J, nb)) return VX_EINVAL;
    if (!y || !pattern || !person || !item || !workspace) return VX_EINVAL;
    if (ws_floats < gf_ws_floats(nb, (int)cfg->J)) return VX_EINVAL;
    const int K = (int)cfg->K, J = (int)cfg->J;
    const GfPlan p = gf_plan(nb);
    hipLaunchKernelGGL(k_fit_cdm, dim3((unsigned)p.n_blocks), dim3(256), 0, (hipStream_t)hs, y, rows, nb, K, J, (int)dino, q, pattern, g_un,
                       s_un, person, workspace, p.n_units, p.units_per_block);
    return grid_fit_finish(p, J, workspace, item, hs);
}

// Point estimates (k_grid_point.hip): ML / MAP / WLE by Fisher scoring, a person's row held on chip; no workspace
static bool point_number_ok(float v) { return v > 0.f && v < INFINITY; }

int vx_grid_point_irt(const vx_irt_cfg* cfg, const uint8_t* y, const int64_t* rows, int64_t nb, const float* theta0, const float* a,
                      const float* b, const float* c_un, const float* d_un, int32_t method, int32_t max_iter, float tol, float bound,
                      float step_cap, float* theta_hat, float* info, int32_t* status, int32_t* iters, void* hs) {
    if (!irt_items_ok(cfg, 4, GF_MAXD, a, b, c_un, d_un) || !grid_point_shape_ok(cfg->J, nb)) return VX_EINVAL;
    if (method != GPT_ML && method != GPT_MAP && method != GPT_WLE) return VX_EINVAL;
    if ((method == GPT_WLE && cfg->D != 1) || max_iter < 1 || max_iter > GPT_MAX_ITERS) return VX_EINVAL;
    if (!point_number_ok(tol) || !point_number_ok(bound) || !point_number_ok(step_cap)) return VX_EINVAL;
    if (!y || !theta0 || !theta_hat || !info || !status || !iters) return VX_EINVAL;
    const int D = (int)cfg->D, J = (int)cfg->J, map = method == GPT_MAP ? 1 : 0;
    const GfPlan p = gf_plan(nb);
    // the instances: (MODEL, 1, WLE) and (MODEL, 1, plain) for D = 1; (MODEL, 3, plain) beyond, where a 1PL cannot be
    return with_irt_model(cfg->model, [&](auto m) -> int {
        constexpr int M = decltype(m)::value;
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)p.n_blocks), dim3(256), 0, (hipStream_t)hs, y, rows, nb, D, J, cfg->Dc, theta0, a, b,
                               c_un, d_un, map, (int)max_iter, tol, bound, step_cap, theta_hat, info, status, iters, p.n_units,
                               p.units_per_block);
        };
        if (method == GPT_WLE) launch(k_point_irt<M, 1, true>);
        else if (D == 1) launch(k_point_irt<M, 1, false>);
        else launch(k_point_irt<(M == 1 ? 2 : M), 3, false>);
        VX_CHECK_LAUNCH();
        return VX_OK;
    });
}

// Summed-score tables (k_sumscore.hip): the Lord-Wingersky recursion behind S-X2 and the score table, and the observed tables
static bool sumscore_shape_ok(int32_t Js, int32_t G) { return Js >= 1 && Js <= SS_MAXJ && G >= 1 && G <= SS_MAXG; }
static bool sumscore_data_ok(int64_t nb, int32_t J, int32_t Js) {
    return nb >= 0 && nb <= ((int64_t)1 << 40) && J >= 1 && J <= SS_MAXJ_ALL && Js >= 1 && Js <= SS_MAXJ && Js <= J;
}

int64_t vx_sumscore_model_workspace_floats(int32_t Js, int32_t G) {
    if (!sumscore_shape_ok(Js, G)) return VX_EINVAL;
    return ss_ws_floats(Js, G);
}

static void sumscore_launch(bool leave, const SsPlan& p, int n_waves, hipStream_t st, const float* p1, const float* p0, const float* logw,
                            int Js, int G, float* out1, float* out0) {
    const dim3 grid((unsigned)((n_waves + SS_WAVES - 1) / SS_WAVES)), block(64 * SS_WAVES);
#define LAUNCH_SS(R)                                                                                                             \
    do {                                                                                                                         \
        if (leave) hipLaunchKernelGGL((k_sumscore<R, true>), grid, block, 0, st, p1, p0, logw, Js, G, p.chunk, p.n_chunks, out1, out0); \
        else hipLaunchKernelGGL((k_sumscore<R, false>), grid, block, 0, st, p1, p0, logw, Js, G, p.chunk, p.n_chunks, out1, out0);      \
    } while (0)
    if (p.R == 1) { LAUNCH_SS(1); } else if (p.R == 2) { LAUNCH_SS(2); } else if (p.R == 4) { LAUNCH_SS(4); }
    else if (p.R == 8) { LAUNCH_SS(8); } else { LAUNCH_SS(16); }
#undef LAUNCH_SS
}

int vx_sumscore_model(const float* p1, const float* p0, const float* logw, int32_t Js, int32_t G, float* e1, float* e0, float* dist,
                      float* workspace, int64_t ws_floats, void* hs) {
    if (!sumscore_shape_ok(Js, G) || !p1 || !p0 || !logw || !e1 || !e0 || !workspace) return VX_EINVAL;
    if (ws_floats < ss_ws_floats(Js, G)) return VX_EINVAL;
    hipStream_t st = (hipStream_t)hs;
    const SsPlan p = ss_plan(Js, G);
    const int64_t len = (int64_t)Js * (Js + 1);
    float* slabs1 = workspace;
    float* slabs0 = workspace + p.n_chunks * len;
    sumscore_launch(true, p, Js * p.n_chunks, st, p1, p0, logw, Js, G, slabs1, slabs0);
    VX_CHECK_LAUNCH();
    int rc = vx_reduce_slabs(slabs1, p.n_chunks, len, 1.0f, e1, hs);
    if (rc) return rc;
    rc = vx_reduce_slabs(slabs0, p.n_chunks, len, 1.0f, e0, hs);
    if (rc) return rc;
    if (dist) {
        // nothing left out: one wave a node, so that the G vectors spread over the chip
        SsPlan pd = p;
        pd.chunk = 1;
        pd.n_chunks = G;
        sumscore_launch(false, pd, G, st, p1, p0, logw, Js, G, dist, nullptr);
        VX_CHECK_LAUNCH();
    }
    return VX_OK;
}

int vx_sumscore_persons(const uint8_t* y, const int64_t* rows, int64_t nb, int32_t J, const int32_t* items, int32_t Js, int32_t* score,
                        void* hs) {
    if (!sumscore_data_ok(nb, J, Js) || !y || !score) return VX_EINVAL;
    if (nb == 0) return VX_OK;
    int64_t blocks = (nb + 3) / 4;
    const int64_t cap = (int64_t)num_cu() * 16;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(k_sumscore_persons, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)hs, y, rows, nb, (int)J, items, (int)Js, score);
    VX_CHECK_LAUNCH();
    return VX_OK;
}

int vx_sumscore_observed(const uint8_t* y, const int64_t* rows, int64_t nb, int32_t J, const int32_t* items, int32_t Js,
                         const int32_t* score, int32_t* o1, void* hs) {
    if (!sumscore_data_ok(nb, J, Js) || !y || !o1 || (nb > 0 && (!rows || !score))) return VX_EINVAL;
    hipStream_t st = (hipStream_t)hs;
    if (hipMemsetAsync(o1, 0, sizeof(int32_t) * (size_t)Js * (size_t)(Js + 1), st) != hipSuccess) return VX_EINVAL;
    if (nb == 0) return VX_OK;
    // chunks of at least 64 persons: the integer sums do not depend on the chunking
    int64_t per_block = (nb + SS_OBS_MAX_BLOCKS - 1) / SS_OBS_MAX_BLOCKS;
    if (per_block < 64) per_block = 64;
    const int64_t blocks = (nb + per_block - 1) / per_block;
    hipLaunchKernelGGL(k_sumscore_observed, dim3((unsigned)blocks), dim3(SS_OBS_THREADS), 0, st, y, rows, nb, (int)J, items, (int)Js,
                       score, o1, per_block);
    VX_CHECK_LAUNCH();
    return VX_OK;
}

// Pairwise 2 x 2 tables (k_pair_tables.hip): u^T u, u^T z, z^T u, z^T z over persons on the int8 MFMA, no workspace
static bool pair_tables_shape_ok(int64_t nb, int32_t J) { return J >= 1 && J <= PT_MAXJ && nb >= 1 && nb <= (int64_t)INT32_MAX; }

int64_t vx_pair_tables_workspace_ints(int64_t nb, int32_t J) {
    if (!pair_tables_shape_ok(nb, J)) return VX_EINVAL;
    return 0;
}

int64_t vx_pair_tables_chunks(int64_t nb, int32_t J) {
    if (!pair_tables_shape_ok(nb, J)) return VX_EINVAL;
    return pt_plan(nb, (int)J).n_chunks;
}

int vx_pair_tables(const uint8_t* y, const int64_t* rows, int64_t nb, int32_t J, int32_t* n11, int32_t* n10, int32_t* n01, int32_t* n00,
                   int32_t* workspace, int64_t ws_ints, void* hs) {
    if (!pair_tables_shape_ok(nb, J) || !y || !n11 || !n10 || !n01 || !n00 || ws_ints < 0) return VX_EINVAL;
    (void)workspace;
    hipStream_t st = (hipStream_t)hs;
    const size_t bytes = sizeof(int32_t) * (size_t)J * (size_t)J;
    for (int32_t* t : {n11, n10, n01, n00})
        if (hipMemsetAsync(t, 0, bytes, st) != hipSuccess) return VX_EINVAL;
    const PtPlan p = pt_plan(nb, (int)J);
    const dim3 grid((unsigned)(p.n_bp * p.n_chunks));
    // a dword a lane where the four items of a dword lie in one row and y is aligned, bytes where not
    if ((J & 3) == 0 && ((uintptr_t)y & 3) == 0)
        hipLaunchKernelGGL(k_pair_tables<true>, grid, dim3(PT_THREADS), 0, st, y, rows, nb, (int)J, p.groups, p.n_stages,
                           p.stages_per_chunk, n11, n10, n01, n00);
    else
        hipLaunchKernelGGL(k_pair_tables<false>, grid, dim3(PT_THREADS), 0, st, y, rows, nb, (int)J, p.groups, p.n_stages,
                           p.stages_per_chunk, n11, n10, n01, n00);
    VX_CHECK_LAUNCH();
    if (p.groups > 1) {
        hipLaunchKernelGGL(k_pair_tables_mirror, dim3(grid_1d((int64_t)J * J, 256)), dim3(256), 0, st, (int)J, n11, n10, n01, n00);
        VX_CHECK_LAUNCH();
    }
    return VX_OK;
}

// ------------------------------------------------------------------------------------------------
// Bernoulli-guide DINA / DINO with the score-function estimator (VCDM / VaeCDM, vi.py:726-816): k_cdm_sf.hip
static bool cdm_sf_cfg_ok(const vx_hodina_cfg* cfg) { return cfg && cfg->K >= 1 && cfg->K <= CS_MAXK && cfg->J >= 1 && cfg->J <= 4096; }
static int cdm_sf_blocks(int64_t nb) {
    const int64_t n_groups = (nb + 63) / 64;
    int64_t blocks = (n_groups + CS_THREADS / 64 - 1) / (CS_THREADS / 64);
    const int64_t cap = (int64_t)num_cu() * 4;
    if (blocks > cap) blocks = cap;
    return (int)(blocks < 1 ? 1 : blocks);
}

int64_t vx_cdm_sf_workspace_floats(const vx_hodina_cfg* cfg, int64_t nb) {
    if (!cdm_sf_cfg_ok(cfg) || nb < 0) return VX_EINVAL;
    return (int64_t)cdm_sf_blocks(nb) * 4 * cfg->J;
}

int vx_cdm_sf_grad(const vx_hodina_cfg* cfg, int32_t dino, int32_t clamp_t, float prior_p, const uint8_t* y,
                   const int64_t* rows, int64_t nb, int64_t gid0, const float* q, const float* g_un, const float* s_un,
                   const float* u, const uint8_t* attr_in, float* baseline, float base_beta, int32_t base_by_row, float* gu,
                   float* log_r, uint8_t* attr_out, float* gitem, float* workspace, void* hs) {
    if (!cdm_sf_cfg_ok(cfg) || !y || !q || !g_un || !s_un || !u || !gu || !log_r || !gitem || !workspace || nb < 0)
        return VX_EINVAL;
    const int blocks = cdm_sf_blocks(nb);
    CdmSfDims dm;
    dm.K = cfg->K; dm.J = cfg->J; dm.dino = dino ? 1 : 0; dm.clamp_t = clamp_t ? 1 : 0; dm.scale = cfg->scale; dm.nb = nb;
    const float pc = fminf(fmaxf(prior_p, VX_EPS32), 1.0f - VX_EPS32);        // Bernoulli(probs).log_prob clamps (vi.py:753: 1.5)
    dm.lp1 = logf(pc); dm.lp0 = log1pf(-pc);
    dm.base_beta = base_beta; dm.base_by_row = base_by_row ? 1 : 0;
    dm.step_dev = cfg->step_dev;
    hipStream_t st = (hipStream_t)hs;
    const size_t lds = (size_t)cfg->J * (4 * sizeof(float) + 4 * sizeof(int) + sizeof(uint32_t));
    int rc = set_lds(k_cdm_sf, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(k_cdm_sf, dim3(blocks), dim3(CS_THREADS), lds, st, dm, y, rows, gid0, u, attr_in, cfg->seed, cfg->step,
                       cfg->stream, q, g_un, s_un, baseline, gu, log_r, attr_out, (int*)workspace);
    VX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_cdm_sf_items, dim3((cfg->J + 127) / 128), dim3(128), 0, st, (int)cfg->J, blocks, cfg->scale,
                       (const int*)workspace, g_un, s_un, gitem);
    VX_CHECK_LAUNCH();
    return VX_OK;
}

int vx_loo_baseline(const float* lr_all, int32_t S, int64_t nb, int32_t s, float* out, void* hs) {
    if (!lr_all || !out || S < 2 || s < 0 || s >= S || nb < 0) return VX_EINVAL;
    if (nb == 0) return VX_OK;
    hipLaunchKernelGGL(k_loo_baseline, dim3(grid_1d(nb, 256)), dim3(256), 0, (hipStream_t)hs, lr_all, (int)S, nb, (int)s, out);
    VX_CHECK_LAUNCH();
    return VX_OK;
}

static bool bin_enc_cfg_ok(const vx_hodina_cfg* cfg) {
    return cfg && cfg->K >= 1 && cfg->K <= CS_MAXK && cfg->H >= 1 && cfg->H <= 128 && cfg->J >= 1;
}
static void bin_enc_plan(const vx_hodina_cfg* cfg, int64_t nb, int& nblk, int& n_jg, int& n_prf) {
    int64_t b = (nb + 3) / 4;
    if (b > 1024) b = 1024;
    nblk = (int)(b < 1 ? 1 : b);
    n_jg = (cfg->J + FC1_JG - 1) / FC1_JG;
    const int64_t n_ptiles = (nb + ENC_P - 1) / ENC_P;
    int64_t f = num_cu() / n_jg; if (f < 1) f = 1;
    n_prf = (int)(n_ptiles < f ? n_ptiles : f); if (n_prf < 1) n_prf = 1;
}

int64_t vx_bin_enc_param_floats(const vx_hodina_cfg* cfg) {
    if (!bin_enc_cfg_ok(cfg)) return VX_EINVAL;
    return (int64_t)cfg->H * cfg->J + cfg->H + (int64_t)cfg->K * cfg->H + cfg->K;
}

int vx_bin_enc_forward(const vx_hodina_cfg* cfg, const uint8_t* y, const int64_t* rows, int64_t nb, const float* W1,
                       const float* b1, const float* W2, const float* b2, float* h, float* u, void* hs) {
    if (!bin_enc_cfg_ok(cfg) || !y || !W1 || !b1 || !W2 || !b2 || !h || !u || nb < 0) return VX_EINVAL;
    if (nb == 0) return VX_OK;
    const int ppb = cfg->H <= 64 ? 4 : 2;                              // persons per block: 256 / hidden slots
    int64_t blocks = (nb + ppb - 1) / ppb;
    if (blocks > (int64_t)num_cu() * 8) blocks = (int64_t)num_cu() * 8;
    if (cfg->H <= 64)
        hipLaunchKernelGGL(k_bin_enc_fwd<64>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)hs, (int)cfg->K, (int)cfg->J,
                           (int)cfg->H, nb, y, rows, W1, b1, W2, b2, h, u);
    else
        hipLaunchKernelGGL(k_bin_enc_fwd<128>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)hs, (int)cfg->K, (int)cfg->J,
                           (int)cfg->H, nb, y, rows, W1, b1, W2, b2, h, u);
    VX_CHECK_LAUNCH();
    return VX_OK;
}

int64_t vx_bin_enc_bwd_workspace_floats(const vx_hodina_cfg* cfg, int64_t nb) {
    if (!bin_enc_cfg_ok(cfg) || nb < 0) return VX_EINVAL;
    int nblk, n_jg, n_prf;
    bin_enc_plan(cfg, nb, nblk, n_jg, n_prf);
    const int64_t H = cfg->H, J = cfg->J, K = cfg->K;
    return nb * H + (int64_t)nblk * (K * H + K) + (int64_t)n_prf * (H * J + H) + 8;          // ghpre | head slabs | fc1 slabs
}

int vx_bin_enc_backward(const vx_hodina_cfg* cfg, const uint8_t* y, const int64_t* rows, int64_t nb, const float* W2,
                        const float* h, const float* gu, float* genc, float* workspace, void* hs) {
    if (!bin_enc_cfg_ok(cfg) || !y || !W2 || !h || !gu || !genc || !workspace || nb < 0) return VX_EINVAL;
    int nblk, n_jg, n_prf;
    bin_enc_plan(cfg, nb, nblk, n_jg, n_prf);
    const int64_t H = cfg->H, J = cfg->J, K = cfg->K;
    const int64_t lenh = K * H + K, lenf = H * J + H;
    float* ghpre = workspace;
    float* slabs_h = ghpre + nb * H;
    float* slabs_f = slabs_h + (int64_t)nblk * lenh;
    hipStream_t st = (hipStream_t)hs;
    hipError_t he = hipMemsetAsync(slabs_h, 0, sizeof(float) * (size_t)(nblk * lenh + n_prf * lenf), st);
    if (he != hipSuccess) return (int)he;
    if (nb > 0) {
        if (H <= 64) hipLaunchKernelGGL(k_bin_enc_bwd_small<64>, dim3(nblk), dim3(256), 0, st, (int)K, (int)H, nb, W2, h, gu, ghpre, slabs_h);
        else hipLaunchKernelGGL(k_bin_enc_bwd_small<128>, dim3(nblk), dim3(256), 0, st, (int)K, (int)H, nb, W2, h, gu, ghpre, slabs_h);
        VX_CHECK_LAUNCH();
        EncDims dm;
        dm.D = 1; dm.J = cfg->J; dm.H = cfg->H; dm.Hp = (cfg->H + 31) / 32 * 32; dm.DS = 3; dm.T = 1; dm.nb = nb;
        // (a small batch: 128 items a workgroup, the form the multivariate guide's small batches take above)
        const int rc = fc1_bwd_person_major(dm, fc1_small_batch(dm.Hp, n_jg, n_prf), n_jg, n_prf, y, rows, ghpre, slabs_f, lenf, 0, st);
        if (rc) return rc;
    }
    // flat layout = nn.Linear order of BinEncoder (vi.py:462-463): [W1 | b1 | W2 | b2]; ghpre already is d LOSS
    int rc2 = vx_reduce_slabs(slabs_f, n_prf, lenf, 1.0f, genc, hs);
    if (rc2) return rc2;
    return vx_reduce_slabs(slabs_h, nblk, lenh, 1.0f, genc + lenf, hs);
}


// ------------------------------------------------------------------------------------------------
// synthetic response matrices (k_synth.hip): benchmark / test input with the reference generators' distributions
int vx_synth_irt(const vx_irt_cfg* cfg, int64_t nb, int64_t gid0, const float* x_in, const float* a, const float* b,
                 const float* c, const float* d, float missing, uint8_t* y, float* x_out, void* hs) {
    if (!cfg || cfg->D < 1 || cfg->D > 128 || cfg->J < 1 || cfg->model < VX_IRT_1PL || cfg->model > VX_IRT_4PL || !b || !y ||
        nb < 0 || missing < 0.f || missing >= 1.f)
        return VX_EINVAL;
    if (cfg->model >= VX_IRT_2PL && !a) return VX_EINVAL;
    if (cfg->model >= VX_IRT_3PL && !c) return VX_EINVAL;
    if (cfg->model == VX_IRT_4PL && !d) return VX_EINVAL;
    if (cfg->model == VX_IRT_1PL && cfg->D != 1) return VX_EINVAL;
    if (nb == 0) return VX_OK;
    int64_t blocks = (nb + SY_P - 1) / SY_P;
    if (blocks > (int64_t)num_cu() * 8) blocks = (int64_t)num_cu() * 8;
    const size_t lds = sizeof(float) * SY_P * (size_t)cfg->D;
    int rc = set_lds(k_synth_irt, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(k_synth_irt, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)hs, (int)cfg->model, (int)cfg->D,
                       (int)cfg->J, cfg->Dc, nb, gid0, x_in, a, b, c, d, missing, cfg->seed, y, x_out);
    VX_CHECK_LAUNCH();
    return VX_OK;
}

int vx_synth_cdm(const vx_hodina_cfg* cfg, int32_t dino, int32_t hodina, float attr_p, int64_t nb, int64_t gid0, const float* q,
                 const float* g, const float* s, const float* lam0, const float* lam1, float missing, uint8_t* y,
                 uint8_t* attr_out, float* theta_out, void* hs) {
    if (!cfg || cfg->K < 1 || cfg->K > 16 || cfg->J < 1 || !q || !g || !s || !y || nb < 0 || missing < 0.f || missing >= 1.f)
        return VX_EINVAL;
    if (hodina && (!lam0 || !lam1)) return VX_EINVAL;
    if (nb == 0) return VX_OK;
    const size_t lds = sizeof(uint32_t) * (size_t)cfg->J;
    int rc = set_lds(k_synth_cdm, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(k_synth_cdm, dim3(grid_1d(nb, 256)), dim3(256), lds, (hipStream_t)hs, (int)cfg->K, (int)cfg->J,
                       dino ? 1 : 0, hodina ? 1 : 0, attr_p, nb, gid0, q, g, s, lam0, lam1, missing, cfg->seed, y, attr_out,
                       theta_out);
    VX_CHECK_LAUNCH();
    return VX_OK;
}


// ------------------------------------------------------------------------------------------------
// VaeCCDM (vi.py:866-891): SoftmaxEncoder prior over the patterns (k_vaeccdm.hip) + the enumeration of k_hodina.hip
static bool sm_enc_cfg_ok(const vx_hodina_cfg* cfg) {
    return cfg && cfg->K >= 1 && cfg->K <= 10 && cfg->H >= 1 && cfg->H <= 128 && cfg->J >= 1 && cfg->J <= 1024;
}
static int col_parts(int64_t nb) {
    int64_t p = (nb + 255) / 256;
    if (p > 256) p = 256;
    return (int)(p < 1 ? 1 : p);
}

int64_t vx_sm_enc_param_floats(const vx_hodina_cfg* cfg) {
    if (!sm_enc_cfg_ok(cfg)) return VX_EINVAL;
    const int64_t C = (int64_t)1 << cfg->K;
    return (int64_t)cfg->H * cfg->J + cfg->H + C * cfg->H + C;
}

int vx_sm_enc_forward(const vx_hodina_cfg* cfg, const uint8_t* y, const int64_t* rows, int64_t nb, const float* W1,
                      const float* b1, const float* W2, const float* b2, float* h, float* z, void* hs) {
    if (!sm_enc_cfg_ok(cfg) || !y || !W1 || !b1 || !W2 || !b2 || !h || !z || nb < 0) return VX_EINVAL;
    if (nb == 0) return VX_OK;
    const int ppb = cfg->H <= 64 ? 4 : 2;
    int64_t blocks = (nb + ppb - 1) / ppb;
    if (blocks > (int64_t)num_cu() * 8) blocks = (int64_t)num_cu() * 8;
    if (cfg->H <= 64)
        hipLaunchKernelGGL(k_sm_enc_fwd<64>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)hs, 1 << cfg->K, (int)cfg->J,
                           (int)cfg->H, nb, y, rows, W1, b1, W2, b2, h, z);
    else
        hipLaunchKernelGGL(k_sm_enc_fwd<128>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)hs, 1 << cfg->K, (int)cfg->J,
                           (int)cfg->H, nb, y, rows, W1, b1, W2, b2, h, z);
    VX_CHECK_LAUNCH();
    return VX_OK;
}

int64_t vx_col_reduce_workspace_floats(int64_t nb, int32_t C) { return (nb < 0 || C < 1) ? VX_EINVAL : (int64_t)col_parts(nb) * C; }

int vx_col_reduce(int32_t mode, const float* v, int64_t nb, int32_t C, const float* shift, float* out, float* workspace,
                  void* hs) {
    if (mode < 0 || mode > 2 || !v || !out || !workspace || nb < 1 || C < 1 || (mode == 1 && !shift)) return VX_EINVAL;
    const int np = col_parts(nb);
    hipLaunchKernelGGL(k_col_part, dim3(np), dim3(256), 0, (hipStream_t)hs, (int)mode, v, nb, (int)C, shift, workspace);
    VX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_col_final, dim3((C + 127) / 128), dim3(128), 0, (hipStream_t)hs, (int)mode, (const float*)workspace, np,
                       (int)C, out);
    VX_CHECK_LAUNCH();
    return VX_OK;
}

int64_t vx_vaeccdm_workspace_floats(const vx_hodina_cfg* cfg, int64_t nb) { return vx_hodina_workspace_floats(cfg, nb); }

int vx_vaeccdm_grad(const vx_hodina_cfg* cfg, int32_t dino, const uint8_t* y, const int64_t* rows, int64_t nb, const float* q,
                    const float* g_un, const float* s_un, const float* z, const float* off, float* elbo, float* gla,
                    float* gitem, float* workspace, void* hs) {
    if (!hodina_cfg_ok(cfg) || !y || !q || !g_un || !s_un || !z || !off || !elbo || !gla || !gitem || !workspace || nb < 0)
        return VX_EINVAL;
    const int blocks = hodina_blocks(nb);
    HoDinaDims dm;
    dm.K = cfg->K; dm.J = cfg->J; dm.C = 1 << cfg->K; dm.scale = cfg->scale; dm.nb = nb;
    dm.uniform_prior = 2; dm.dino = dino ? 1 : 0; dm.unmasked = 1;
    dm.gsz = hodina_gsz(nb);
    const int len = 2 * cfg->J + 2 * cfg->K;
    const size_t lds = hodina_lds_bytes(dm.C, len);
    hipStream_t st = (hipStream_t)hs;
    const int logcpl = cfg->K <= 8 ? 2 : (cfg->K == 9 ? 3 : 4);
    const int jpl = (cfg->J + 63) / 64;
    const float* nul = nullptr;
    float* fnul = nullptr;
#define LAUNCH_VC(L, JP)                                                                                      \
    hipLaunchKernelGGL((k_hodina<L, JP>), dim3(blocks), dim3(HD_THREADS), lds, st, dm, y, rows, (int64_t)0, nul, nul, \
                       nul, (uint64_t)0, 0u, 0u, q, nul, nul, g_un, s_un, fnul, fnul, elbo, workspace, z, off, gla)
#define DISPATCH_VC(L)                               \
    if (jpl <= 1) { LAUNCH_VC(L, 1); }               \
    else if (jpl <= 2) { LAUNCH_VC(L, 2); }          \
    else if (jpl <= 4) { LAUNCH_VC(L, 4); }          \
    else if (jpl <= 8) { LAUNCH_VC(L, 8); }          \
    else { LAUNCH_VC(L, 16); }
    if (logcpl == 2) { DISPATCH_VC(2) } else if (logcpl == 3) { DISPATCH_VC(3) } else { DISPATCH_VC(4) }
#undef DISPATCH_VC
#undef LAUNCH_VC
    VX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_reduce_slabs, dim3(grid_1d(2 * cfg->J, 64)), dim3(256), 0, st, workspace, (int64_t)blocks,
                       (int64_t)len, (int64_t)(2 * cfg->J), -1.0f, gitem);
    VX_CHECK_LAUNCH();
    return VX_OK;
}

static void sm_bwd_plan(const vx_hodina_cfg* cfg, int64_t nb, int& n_rs, int& n_jg, int& n_prf) {
    int64_t r = (nb + 511) / 512;
    if (r > 32) r = 32;
    n_rs = (int)(r < 1 ? 1 : r);
    n_jg = (cfg->J + FC1_JG - 1) / FC1_JG;
    const int64_t n_ptiles = (nb + ENC_P - 1) / ENC_P;
    int64_t f = num_cu() / n_jg; if (f < 1) f = 1;
    n_prf = (int)(n_ptiles < f ? n_ptiles : f); if (n_prf < 1) n_prf = 1;
}

int64_t vx_sm_enc_bwd_workspace_floats(const vx_hodina_cfg* cfg, int64_t nb) {
    if (!sm_enc_cfg_ok(cfg) || nb < 0) return VX_EINVAL;
    int n_rs, n_jg, n_prf;
    sm_bwd_plan(cfg, nb, n_rs, n_jg, n_prf);
    const int64_t H = cfg->H, J = cfg->J, C = (int64_t)1 << cfg->K;
    return nb * H + (int64_t)n_rs * (C * H + C) + (int64_t)n_prf * (H * J + H) + 8;
}

int vx_sm_enc_backward(const vx_hodina_cfg* cfg, const uint8_t* y, const int64_t* rows, int64_t nb, const float* W2,
                       const float* h, const float* z, const float* off, const float* T, float* gla, float* genc,
                       float* workspace, void* hs) {
    if (!sm_enc_cfg_ok(cfg) || !y || !W2 || !h || !z || !off || !T || !gla || !genc || !workspace || nb < 0) return VX_EINVAL;
    int n_rs, n_jg, n_prf;
    sm_bwd_plan(cfg, nb, n_rs, n_jg, n_prf);
    const int64_t H = cfg->H, J = cfg->J, C = (int64_t)1 << cfg->K;
    const int64_t lenh = C * H + C, lenf = H * J + H;
    float* ghpre = workspace;
    float* slabs_h = ghpre + nb * H;
    float* slabs_f = slabs_h + (int64_t)n_rs * lenh;
    hipStream_t st = (hipStream_t)hs;
    hipError_t he = hipMemsetAsync(slabs_h, 0, sizeof(float) * (size_t)(n_rs * lenh + n_prf * lenf), st);
    if (he != hipSuccess) return (int)he;
    if (nb > 0) {
        hipLaunchKernelGGL(k_vaeccdm_gz, dim3(grid_1d(nb * C, 256)), dim3(256), 0, st, z, off, T, nb, (int)C, gla);
        VX_CHECK_LAUNCH();
        const int ppb = H <= 64 ? 4 : 2;
        int64_t blocks = (nb + ppb - 1) / ppb;
        if (blocks > (int64_t)num_cu() * 8) blocks = (int64_t)num_cu() * 8;
        if (H <= 64) hipLaunchKernelGGL(k_sm_enc_bwd_h<64>, dim3((unsigned)blocks), dim3(256), 0, st, (int)C, (int)H, nb, W2, h, (const float*)gla, ghpre);
        else hipLaunchKernelGGL(k_sm_enc_bwd_h<128>, dim3((unsigned)blocks), dim3(256), 0, st, (int)C, (int)H, nb, W2, h, (const float*)gla, ghpre);
        VX_CHECK_LAUNCH();
        if (H <= 64)
            hipLaunchKernelGGL(k_sm_enc_bwd_w<64>, dim3((unsigned)((C + 63) / 64), (unsigned)n_rs), dim3(256), 0, st, (int)C, (int)H, nb, h,
                               (const float*)gla, slabs_h);
        else
            hipLaunchKernelGGL(k_sm_enc_bwd_w<128>, dim3((unsigned)((C + 63) / 64), (unsigned)n_rs), dim3(256), 0, st, (int)C, (int)H, nb, h,
                               (const float*)gla, slabs_h);
        VX_CHECK_LAUNCH();
        EncDims dm;
        dm.D = 1; dm.J = cfg->J; dm.H = cfg->H; dm.Hp = (cfg->H + 31) / 32 * 32; dm.DS = 3; dm.T = 1; dm.nb = nb;
        // (a small batch: 128 items a workgroup, the form the multivariate guide's small batches take above)
        const int rc = fc1_bwd_person_major(dm, fc1_small_batch(dm.Hp, n_jg, n_prf), n_jg, n_prf, y, rows, ghpre, slabs_f, lenf, 0, st);
        if (rc) return rc;
    }
    // gz / ghpre are d ELBO: loss gradients = -(.)   flat layout [W1 | b1 | W2 | b2] (SoftmaxEncoder, vi.py:477-478)
    int rc2 = vx_reduce_slabs(slabs_f, n_prf, lenf, -1.0f, genc, hs);
    if (rc2) return rc2;
    return vx_reduce_slabs(slabs_h, n_rs, lenh, -1.0f, genc + lenf, hs);
}

}  // extern "C"
