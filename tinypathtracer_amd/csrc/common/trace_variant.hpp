// trace_variant.hpp -- the k_trace variant space, written once: what each family
// fixes, the key that names one variant, the rule that picks a launch's key and a
// variant's LDS layout.  No HIP: trace.hip instantiates and launches from it,
// launch_plan.cpp plans with it, tests/sanitize/host_check.cpp "variant" checks it.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <type_traits>

#ifndef TPT_TRACE_WAVES
#define TPT_TRACE_WAVES 5   // min waves per SIMD requested from the register allocator
#endif
#ifndef TPT_TRACE_WAVES_IS
// The env importance-sampling variants (A15) carry the env sample's state across
// the shading pass: at 96 VGPRs (5 waves) they spilled 121 VGPRs to scratch;
// 4 waves give them 128.
#define TPT_TRACE_WAVES_IS 4
#endif
#ifndef TPT_TRACE_WAVES_PAIR
// pair-mode (delta-light) variants: at 5 waves (96 VGPRs) they spilled 38 VGPRs;
// C3 4096 spp, 4 waves: +6.4 % (7,220 -> 7,685 Mrays/s, 2 interleaved reps)
#define TPT_TRACE_WAVES_PAIR 4
#endif
#ifndef TPT_TRACE_WAVES_DRAIN
// DRAIN variants (launches that cannot fill the chip: a few waves per SIMD anyway)
#define TPT_TRACE_WAVES_DRAIN 4
#endif
#ifndef TPT_TRACE_WAVES_QUAD
#define TPT_TRACE_WAVES_QUAD 4   // four lanes per pixel (k_trace QUAD)
#endif

// WGW: the waves of a k_trace workgroup (1, 2 or 4; block size 64 * WGW), one
// shape per variant family ("Workgroup shape").  A wave's
// tile does not depend on it.  A workgroup's LDS and its waves' slots are handed
// on only when its last wave ends, so a smaller workgroup returns the slots of
// waves that end before their tile's siblings sooner.
// -DTPT_WG_WAVES=N (EXTRA) builds every family at N waves: 4 is the shape before
// WGW existed, for an A/B library from the same tree.
#ifdef TPT_WG_WAVES
#define TPT_WGW(n) TPT_WG_WAVES
#else
#define TPT_WGW(n) n
#endif
// Measured: one lane per pixel at one wave, C2 +2.6 %; the other families
// keep four waves until their own configurations are measured.
#define TPT_WGW_LANE TPT_WGW(1)    // one lane per pixel, ordered traversal
#define TPT_WGW_DRAIN TPT_WGW(1)   // the same, drained launches
#define TPT_WGW_PAIR TPT_WGW(4)    // pair mode
#define TPT_WGW_IS TPT_WGW(4)      // env importance sampling (pair mode or one lane)
#define TPT_WGW_QUAD TPT_WGW(4)    // four lanes per pixel
#define TPT_WGW_REF TPT_WGW(4)     // the reference's visit order
#ifndef TPT_MTL_LDS_MAX
#define TPT_MTL_LDS_MAX 2048   // bytes: material tables up to 64 entries go to LDS
#endif

namespace tpt {

// The first six are the families of tpt_debug_trace_wg_waves, in its order.  The last two are
// the env-IS forms of the rows they are named after: rows of their own, for they fix other numbers.
enum TraceFamily : int { TF_LANE, TF_DRAIN, TF_PAIR, TF_IS, TF_QUAD, TF_REF, TF_IS_PAIR, TF_REF_IS, kTraceFamilies };
constexpr int kTracePublicFamilies = 6;

struct TraceFamilyInfo {
    int wgw;               // waves per workgroup
    int waves;             // waves per SIMD: __launch_bounds__, and the workgroups that fill a CU
    int lds_waves;         // waves per SIMD whose share of the CU's LDS a workgroup may use
    int lanes;             // lanes per pixel: 1, 2 (pair mode) or 4
    int tile_w, tile_rows; // pixels of a tile (four waves)
    bool env_is, ordered;
};
// DRAIN keeps the one-lane LDS budget: a scene's layout does not depend on the launch size.
// TF_REF_IS is compiled for 4 waves per SIMD but lays its LDS out for 5; recorded as found
// (equal numbers would change its occupancy or its LDS levels, which needs a measurement).
inline constexpr TraceFamilyInfo kTraceFamily[kTraceFamilies] = {
    /* TF_LANE    */ {TPT_WGW_LANE, TPT_TRACE_WAVES, TPT_TRACE_WAVES, 1, 16, 16, false, true},
    /* TF_DRAIN   */ {TPT_WGW_DRAIN, TPT_TRACE_WAVES_DRAIN, TPT_TRACE_WAVES, 1, 16, 16, false, true},
    /* TF_PAIR    */ {TPT_WGW_PAIR, TPT_TRACE_WAVES_PAIR, TPT_TRACE_WAVES_PAIR, 2, 16, 8, false, true},
    /* TF_IS      */ {TPT_WGW_IS, TPT_TRACE_WAVES_IS, TPT_TRACE_WAVES_IS, 1, 16, 16, true, true},
    /* TF_QUAD    */ {TPT_WGW_QUAD, TPT_TRACE_WAVES_QUAD, TPT_TRACE_WAVES_QUAD, 4, 8, 8, false, true},
    /* TF_REF     */ {TPT_WGW_REF, TPT_TRACE_WAVES, TPT_TRACE_WAVES, 1, 16, 16, false, false},
    /* TF_IS_PAIR */ {TPT_WGW_IS, TPT_TRACE_WAVES_IS, TPT_TRACE_WAVES_IS, 2, 16, 8, true, true},
    /* TF_REF_IS  */ {TPT_WGW_REF, TPT_TRACE_WAVES_IS, TPT_TRACE_WAVES, 1, 16, 16, true, false},
};

// One variant: its family and what the scene and the call decide within it.
struct TraceKey {
    TraceFamily family;
    bool deep;       // path records for max_depth up to 64 (else 8)
    bool lights;     // 5-word path records (else 2 packed words)
    bool mtl_lds;    // material table in LDS
    bool wide_ids;   // 32-bit node ids on the traversal stack (else 16-bit)
    bool noemit;     // no triangle emits: the probe's traversal phases are compiled out
};
constexpr int kTraceKeyBits = 8;
constexpr unsigned trace_key_pack(const TraceKey& k) {
    return (unsigned)k.family | k.deep << 3 | k.lights << 4 | k.mtl_lds << 5 | k.wide_ids << 6 | k.noemit << 7;
}
constexpr TraceKey trace_key_unpack(unsigned p) {
    return {(TraceFamily)(p & 7), (p >> 3 & 1) != 0, (p >> 4 & 1) != 0, (p >> 5 & 1) != 0, (p >> 6 & 1) != 0, (p >> 7 & 1) != 0};
}
// The variants that exist as kernels (82 per build).
constexpr bool trace_key_legal(const TraceKey& k) {
    const TraceFamilyInfo& f = kTraceFamily[k.family];
    // the reference order has one general variant: 64 levels of 5 words, global materials, 32-bit ids
    if (!f.ordered && !(k.deep && k.lights && !k.mtl_lds && k.wide_ids)) return false;
    // pair mode and env IS keep the direct term (5 words); four lanes run the one-lane logic without delta lights
    if (k.lights ? f.lanes == 4 : (f.lanes == 2 || f.env_is)) return false;
    return !k.noemit || f.lanes == 2;   // NOEMIT is a pair-mode specialisation
}

// Run-ahead (k_trace, TraceArgs credit / ahead_max): when a set's spp is
// cut into several launches, a lane that has run this launch's samples while another lane of
// its wave still owes some goes on with the pixel's next samples, up to ahead_max, instead of
// idling until the wave ends; the pixel's credit plane tells the set's next launch how many
// of its samples are already done.  A pixel's samples still run in order on its own RNG
// stream and sum in the same order, so the frame is bit-identical.  The one-lane
// full-occupancy family's 8-level variants only: the others are compiled without it.  (The
// 64-level variants measured -2.6 % with it at C4, tir at depth 32, where a tile's time is a few
// pixels' long chains and the lanes that run ahead beside them slow those chains down.)
constexpr bool trace_runs_ahead(TraceFamily f, bool deep) { return f == TF_LANE && !deep; }

// The descriptor k_trace is instantiated with.
template <TraceFamily F, int MAXD_, bool LIGHTS_, bool MTL_LDS_, typename StackT_, bool NOEMIT_>
struct TraceVariant {
    static_assert((MAXD_ == 8 || MAXD_ == 64) && (std::is_same_v<StackT_, uint16_t> || std::is_same_v<StackT_, int>));
    static constexpr TraceKey key{F, MAXD_ == 64, LIGHTS_, MTL_LDS_, sizeof(StackT_) == 4, NOEMIT_};
    static_assert(trace_key_legal(key), "no such k_trace variant (trace_key_legal)");
    static constexpr TraceFamilyInfo fam = kTraceFamily[F];
    static_assert(fam.wgw == 1 || fam.wgw == 2 || fam.wgw == 4, "waves per k_trace workgroup: 1, 2 or 4");
    static constexpr int MAXD = MAXD_, WGW = fam.wgw, WAVES = fam.waves;
    static constexpr bool ORDERED = fam.ordered, LIGHTS = LIGHTS_, MTL_LDS = MTL_LDS_, ENVIS = fam.env_is,
                          PAIR = fam.lanes == 2, DRAIN = F == TF_DRAIN, QUAD = fam.lanes == 4, NOEMIT = NOEMIT_;
    // the pruned unwind (below): the 2-word-record variants of the one-lane, DRAIN and four-lane families
    static constexpr bool PRUNE = !LIGHTS_ && ORDERED && !PAIR && !ENVIS;
    // lanes run ahead across a set's sample chunks (trace_runs_ahead below)
    static constexpr bool AHEAD = trace_runs_ahead(F, MAXD_ == 64);
    using StackT = StackT_;
};

// Pruned unwind (k_trace, 2-word records).  The unwind's step is
// L = (1/p) * ((dst + L) * (af * color)).  A level is *clean* when its probe reached no
// emitter (dst is exactly +0), its p is af itself (p-kind 0) and af lies in
// [kPruneAfMin, kPruneAfMax]; the scene is prunable when every baseColor component passes
// prune_color_ok.  Then a clean level maps L = +0 to +0, in IEEE arithmetic without
// contraction:
//   +0 + +0 = +0;
//   +0 * x = +0 for finite x with a clear sign bit, and x = af * color is that: af is
//     positive and at most 2^100, color has a clear sign bit and is at most 2^27, so the
//     product is at most 2^127 and has a clear sign bit (+0 where color is +0 or it underflows);
//   y * +0 = +0 for finite positive y, and y = 1 / af is that for af in [2^-100, 2^100].
// A path that ends with L = +0 (a miss without env map, max_depth) therefore keeps +0 down
// to the deepest level that is not clean, and the unwind may start there.  Every level it
// does run is the same arithmetic on the same inputs.  The p-kinds 1 and 2 (p = -0 / +0, a
// hemisphere sample whose cosine rounds to zero) divide by zero: such a level is never
// clean.  No test input reaches them -- the sample's cosine is at least about 1.5e-5 --
// so the rule for them is conservative and rests on this argument alone.
constexpr float kPruneAfMin = 0x1p-100f, kPruneAfMax = 0x1p100f, kPruneColorCap = 0x1p27f;
// finite, sign bit clear (no -0, no negative NaN) and at most the cap: as bits, one unsigned
// compare (a set sign bit, inf and NaN all lie above the cap's pattern, 2^27 = 0x4d000000)
inline bool prune_color_ok(float c) {
    uint32_t b;
    std::memcpy(&b, &c, sizeof b);
    return b <= 0x4d000000u;
}

constexpr uint32_t kNoProbe = 0x7fffu;   // the packed records' 15-bit probe material id for "the probe hit nothing"
// Path-record words per bounce (k_trace): 2 when the scene has no delta lights
// (atten; material | probe material | p-kind packed), else 5 (atten; material |
// p-kind; direct term x3).  The packed form needs material ids below kNoProbe.
constexpr int rec_words(int n_lights, int n_materials) {
    return (n_lights > 0 || n_materials + 1 >= (int)kNoProbe) ? 5 : 2;
}
// 16-bit node ids: the binary tree's 2F - 1 nodes
constexpr bool trace_small_ids(int n_faces) { return 2 * (size_t)n_faces - 1 <= 65535; }
// the material table (two float4 per material and the Material() slot) goes to LDS
constexpr bool trace_mtl_in_lds(int n_materials) { return (size_t)(n_materials + 1) * 32 <= (size_t)TPT_MTL_LDS_MAX; }
// 5-word records: the reference order's and env IS's variants always, else by rec_words
constexpr bool trace_five_words(bool ref_order, bool env_is, int n_lights, int n_materials) {
    return ref_order || env_is || rec_words(n_lights, n_materials) == 5;
}

// What launch_trace sees of a call and its scene: TPT_FLAG_REF_ORDER, env next-event
// estimation on, the plan's requests (TraceArgs pair, quad, drained), the scene's sizes.
struct TraceSelectIn {
    bool ref_order, env_is, pair, quad, drained;
    int n_lights, n_materials, n_faces, max_depth;
    bool any_emitter;
};
struct TraceSelection {
    TraceKey key;
    const char* error;   // null: key is the variant to launch
};
// The one selection rule.  Pair mode is granted where there are shadow rays to hand
// off (delta lights, or env IS's sample) and the material ids leave kNoProbe free;
// DRAIN only to one-lane ordered launches; four lanes only with 2-word records.
constexpr TraceSelection select_trace_variant(const TraceSelectIn& in) {
    if (in.ref_order) return {{in.env_is ? TF_REF_IS : TF_REF, true, true, false, true, false}, nullptr};
    const bool pair = in.pair && (in.env_is || in.n_lights > 0) && in.n_materials + 1 < (int)kNoProbe;
    TraceKey k{TF_LANE, in.max_depth > 8, trace_five_words(false, in.env_is, in.n_lights, in.n_materials),
               trace_mtl_in_lds(in.n_materials), !trace_small_ids(in.n_faces), pair && !in.any_emitter};
    if (in.env_is) k.family = pair ? TF_IS_PAIR : TF_IS;
    else if (in.quad) k.family = TF_QUAD;
    else if (pair) k.family = TF_PAIR;
    else if (in.drained) k.family = TF_DRAIN;
    return {k, trace_key_legal(k) ? nullptr : "four lanes per pixel need 2-word path records"};
}

// LDS of a variant's workgroup of `wgw` waves: [material table][traversal stack][path records].
struct TraceLds {
    size_t bytes;
    int mtl_offset, stack_offset, rec_offset;
    int stack_slots, rec_levels;   // held in LDS; deeper ones in private memory
};
constexpr size_t kLdsSlack = 512;   // bytes per wave left free in workgroups of fewer than four waves

// The layout within the workgroup's share of the CU's 160 KiB when the CU holds the
// family's lds_waves per SIMD (a 4-wave workgroup's share rounded down to 256 B, times
// wgw / 4).  max_slots / max_levels cap the stack slots and record levels (fit_lds).
inline TraceLds trace_lds_layout(const TraceKey& k, int wgw, int stack_depth, int max_depth, int n_materials,
                                 size_t max_slots = (size_t)-1, size_t max_levels = (size_t)-1) {
    const TraceFamilyInfo& f = kTraceFamily[k.family];
    // Priorities (measured on box): the whole stack (a
    // stack capped at 23 of its 40 slots cost 7 %), then path records up to
    // max_depth (records of long paths in private memory slow the heaviest
    // tiles).
    size_t lds_budget = ((163840 / (size_t)f.lds_waves) & ~(size_t)255) * (size_t)wgw / 4;
    // Smaller workgroups leave kLdsSlack bytes per wave unused.  A layout that fills the
    // CU's LDS exactly (box at one wave: 20 x 8,192 B) was resident only four waves per
    // SIMD deep on the device although the runtime's occupancy query (fit_lds) answered
    // five: C2 -2.8 %; with 512 B per wave of slack +2.6 % ("Workgroup shape").
    if (wgw < 4) lds_budget -= kLdsSlack * (size_t)wgw;
    const size_t row = 64 * (size_t)wgw;   // the workgroup's lanes
    const size_t mtl_bytes = k.mtl_lds ? ((size_t)(n_materials + 1) * 2 * 16 + 127) / 128 * 128 : 0;
    const size_t budget = lds_budget - mtl_bytes;
    const size_t elem = k.wide_ids ? 4 : 2;
    const size_t slot = f.lanes == 4 ? row / 4 * elem : row * elem;   // (quad: four slots per row of lanes)
    const size_t level = (size_t)(k.lights ? 5 : 2) * (f.lanes == 2 ? row / 2 : row) * sizeof(float);
    // The whole stack (capacity + 3 spare slots for the unconditional 4-wide
    // pushes) when the path records of max_depth levels fit beside it.  Else
    // the records first: the ordered walk rarely goes deep (C5: 99 % of visits
    // find <= 5 entries), so the stack keeps as many slots as the records leave,
    // at least 12, and deeper entries spill to private memory.  Measured on C5
    // (44 slots of 32-bit ids): 27 stack slots + 2 record levels 7.63 Grays/s,
    // 19 + 6: 7.97, 12 + 8: 8.20.
    size_t slots = std::min((size_t)stack_depth + 3, max_slots);
    const size_t want = std::min(std::min<size_t>((size_t)max_depth, (budget - 12 * slot) / level), max_levels);
    if (slots * slot + want * level > budget)
        slots = std::min(slots, std::max<size_t>(12, ((budget - want * level) / slot) & ~(size_t)1));   // even
    // the region holds a whole number of slot pairs (quad: of 4-slot rows), rounded to 16 bytes
    const size_t stack = f.lanes == 4 ? ((slots + 3) / 4 * 4 * slot + 15) / 16 * 16
                                      : ((slots + 1) / 2 * 2 * slot + 15) / 16 * 16;
    const size_t levels = std::min(std::min((budget - stack) / level, (size_t)max_depth), max_levels);
    return {mtl_bytes + stack + levels * level, 0, (int)mtl_bytes, (int)(mtl_bytes + stack), (int)slots, (int)levels};
}

}  // namespace tpt
