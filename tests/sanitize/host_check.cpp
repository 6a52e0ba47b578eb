// host_check.cpp -- CPU-only driver of the host parsers and the wide-tree
// builder for the sanitizer build (tests/sanitize/Makefile, SURVEY.md section 5
// "CPU restatement under ASan/UBSan").  Never built for or run on the GPU box.
//
//   host_check gltf FILE...   load_gltf (host/gltf.cpp, json_lite.hpp)
//   host_check image FILE...  load_image (host/image.cpp: JPEG / PPM)
//   host_check wide N SEED    build_wide_sah (host/wide_bvh.cpp) on N random leaf boxes
//   host_check plan CASE...   plan_launches (host/launch_plan.cpp); CASE is key=value,... (plan_case below);
//                             prints the plan as one JSON object per case
//   host_check plan-sweep N SEED   N random cases, the plan's invariants checked here
//   host_check variant CASE...     the k_trace variant space (common/trace_variant.hpp); CASE is "table", or
//                                  key=value,... with select=1 (select_trace_variant) or layout=1
//                                  (trace_lds_layout) first (variant_case below); one JSON object per case
//   host_check variant-sweep N SEED   plan-sweep's cases and more: every plan's lane mode and workgroup rows
//                                  are those of the variant launch_trace selects for the plan's requests
//   host_check jumps N        N threads make the process's first host_jumps() calls together (host/rng_host.cpp):
//                             each must see the table xorwow_jump_matrices builds serially; "ok", or
//                             "differs <thread> ..." per thread that saw another one and exit status 1
//   host_check parse-threads N [--gltf FILE...] [--image FILE...] [--plan CASE...] [--variant CASE...]
//                             N threads load the scenes and images and run the plan and variant cases at once,
//                             each on its own objects; each must get the serial run's bytes
//
// Prints one line per input: "ok", or "error: <message>" for a parse error
// (the library's exception, which tpt_gltf_load / tpt_env_load turn into a
// status).  Any memory error or undefined behaviour aborts with the
// sanitizer's report instead.
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <random>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../common/rng.hpp"
#include "launch_plan.hpp"
#include "tpt_internal.hpp"

// A launch-plan case as tpt_render_frames hands it to plan_launches: the frame
// and deal (bh derived as the entry point derives it), tpt_params, the scene.
struct PlanCase {
    tpt::PlanInput in;
    std::vector<int32_t> list;
    void finish() {
        in.list = list.data();
        in.list_len = list.size();
        in.bh = in.listed ? tpt::band_list_rows(list.data(), list.size(), in.band_rows, in.height)
                          : tpt::band_height_of(in.height, in.band_rows, in.band_count, in.band_index);
    }
};

// key=value,...: w h rows bc bi list (ids joined by ':', "-" for an empty list) frames | spp flags lanes refill
// leaf spl sets chunks | faces lights mtls resident env_is quad_fits.  Defaults: 16 band rows, one frame, the whole
// frame, 327,680 resident lanes, quad_fits, everything else 0.
static bool plan_case(const std::string& text, PlanCase& c) {
    c.in.resident_lanes = 327680;
    c.in.quad_fits = true;
    size_t at = 0;
    while (at < text.size()) {
        const size_t end = std::min(text.find(',', at), text.size()), eq = text.find('=', at);
        if (eq == std::string::npos || eq >= end) return false;
        const std::string key = text.substr(at, eq - at), val = text.substr(eq + 1, end - eq - 1);
        const long long v = std::atoll(val.c_str());
        if (key == "w") c.in.width = (int32_t)v;
        else if (key == "h") c.in.height = (int32_t)v;
        else if (key == "rows") c.in.band_rows = (int32_t)v;
        else if (key == "bc") c.in.band_count = (int32_t)v;
        else if (key == "bi") c.in.band_index = (int32_t)v;
        else if (key == "frames") c.in.n_frames = (int32_t)v;
        else if (key == "spp") c.in.spp = (int32_t)v;
        else if (key == "flags") c.in.flags = (int32_t)v;
        else if (key == "lanes") c.in.lanes_per_pixel = (int32_t)v;
        else if (key == "refill") c.in.refill = (int32_t)v;
        else if (key == "leaf") c.in.leaf_batch = (int32_t)v;
        else if (key == "spl") c.in.spp_per_launch = (int32_t)v;
        else if (key == "sets") c.in.pipe_sets = (int32_t)v;
        else if (key == "chunks") c.in.pipe_chunks = (int32_t)v;
        else if (key == "faces") c.in.n_faces = (int32_t)v;
        else if (key == "lights") c.in.n_lights = (int32_t)v;
        else if (key == "mtls") c.in.n_materials = (int32_t)v;
        else if (key == "resident") c.in.resident_lanes = (uint64_t)v;
        else if (key == "env_is") c.in.env_is = v != 0;
        else if (key == "quad_fits") c.in.quad_fits = v != 0;
        else if (key == "list") {
            c.in.listed = true;
            for (size_t i = 0; i < val.size() && val != "-";) {
                c.list.push_back((int32_t)std::atoi(val.c_str() + i));
                const size_t colon = val.find(':', i);
                i = colon == std::string::npos ? val.size() : colon + 1;
            }
        } else {
            return false;
        }
        at = end + 1;
    }
    c.finish();
    return true;
}

template <class It, class F>
static void print_list(FILE* f, const char* name, It b, It e, F item) {
    std::fprintf(f, ",\"%s\":[", name);
    for (It i = b; i != e; ++i) {
        if (i != b) std::fprintf(f, ",");
        item(*i);
    }
    std::fprintf(f, "]");
}

static void print_plan(const PlanCase& c, const tpt::LaunchPlan& pl, FILE* f = stdout) {
    if (pl.status != TPT_OK) {
        std::fprintf(f, "{\"status\":%d,\"message\":\"%s\"}\n", (int)pl.status, pl.message);
        return;
    }
    std::fprintf(f, "{\"status\":0,\"bh\":%d,\"pair\":%d,\"pair_kernel\":%d,\"quad\":%d,\"drained\":%d,\"refill\":%d,"
                "\"leaf_kb\":%d,\"xcd_run\":%d,\"wg_rows\":%d,\"nset\":%d,\"chunk\":%d",
                c.in.bh, pl.pair, pl.pair_kernel, pl.quad, pl.drained, pl.refill, pl.leaf_kb, pl.xcd_run, pl.wg_rows,
                pl.nset, pl.chunk);
    print_list(f, "launches", pl.launches.begin(), pl.launches.end(),
               [f](const tpt::PlanLaunch& l) { std::fprintf(f, "[%d,%d]", l.set, l.samples); });
    print_list(f, "order", pl.order.begin(), pl.order.end(), [f](size_t j) { std::fprintf(f, "%zu", j); });
    print_list(f, "set_rows", pl.set_rows, pl.set_rows + pl.nset, [f](int32_t r) { std::fprintf(f, "%d", r); });
    print_list(f, "set_off", pl.set_off, pl.set_off + pl.nset, [f](size_t o) { std::fprintf(f, "%zu", o); });
    print_list(f, "set_list", pl.set_list, pl.set_list + pl.nset, [f](const std::vector<int32_t>& l) {
        std::fprintf(f, "[");
        for (size_t i = 0; i < l.size(); ++i) std::fprintf(f, i ? ",%d" : "%d", l[i]);
        std::fprintf(f, "]");
    });
    std::fprintf(f, "}\n");
}

// The invariants every plan keeps; returns what is broken (null: nothing).
static const char* plan_broken(const PlanCase& c, const tpt::LaunchPlan& pl) {
    const tpt::PlanInput& in = c.in;
    if (pl.nset < 1 || pl.nset > tpt::kMaxPipe || pl.chunk < 1 || pl.chunk > in.spp) return "nset or chunk out of range";
    // every set's samples sum to spp (no launches without rows); inner launches are whole chunks
    std::vector<std::vector<int>> per((size_t)pl.nset);
    for (const tpt::PlanLaunch& l : pl.launches) {
        if (l.set < 0 || l.set >= pl.nset || l.samples < 1) return "launch out of range";
        per[(size_t)l.set].push_back(l.samples);
    }
    for (const std::vector<int>& s : per) {
        long long sum = 0;
        for (size_t i = 0; i < s.size(); ++i) {
            sum += s[i];
            if (i > 0 && i + 1 < s.size() && s[i] != pl.chunk) return "an inner launch is not a whole chunk";
            if (s[i] > pl.chunk) return "a launch is longer than a chunk";
        }
        if (sum != (in.bh > 0 ? in.spp : 0)) return "a set's samples do not sum to spp";
    }
    // the issue order: a permutation of the launches, each set's in plan order (plan order is set by set)
    if (pl.order.size() != pl.launches.size()) return "issue order: wrong length";
    std::vector<int> seen(pl.launches.size(), 0);
    std::vector<long long> last((size_t)pl.nset, -1);
    for (size_t j : pl.order) {
        if (j >= seen.size() || seen[j]++) return "issue order: not a permutation";
        const int k = pl.launches[j].set;
        if ((long long)j < last[(size_t)k]) return "issue order: a set's launches out of order";
        last[(size_t)k] = (long long)j;
    }
    // the sets' rows sum to the call's
    long long rows = 0;
    for (int k = 0; k < pl.nset; ++k) rows += pl.set_rows[k];
    if (rows != in.bh) return "set rows do not sum to bh";
    // an explicit deal over several sets: the shares partition the list and lie back to back behind it
    if (in.listed && pl.nset > 1) {
        std::vector<int32_t> all;
        size_t off = c.list.size();
        for (int k = 0; k < pl.nset; ++k) {
            if (pl.set_off[k] != off) return "set shares are not back to back behind the list";
            off += pl.set_list[k].size();
            all.insert(all.end(), pl.set_list[k].begin(), pl.set_list[k].end());
        }
        std::vector<int32_t> want = c.list;
        std::sort(all.begin(), all.end());
        std::sort(want.begin(), want.end());
        if (all != want) return "set shares do not partition the list";
    }
    return nullptr;
}

// One random case of the sweeps.
static void random_case(std::mt19937& rng, PlanCase& c) {
    auto pick = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
    {
        tpt::PlanInput& in = c.in;
        static const int kRows[] = {1, 4, 8, 16, 32};
        static const int kRes[] = {640, 20480, 327680};
        in.width = rng() % 4 ? pick(4, 400) : pick(400, 4000);
        in.height = rng() % 4 ? pick(1, 300) : pick(300, 2200);
        in.band_rows = kRows[rng() % 5];
        in.n_frames = pick(1, 3);
        const int n_bands = (in.height + in.band_rows - 1) / in.band_rows;
        if (rng() % 3 == 0) {   // an explicit deal: distinct bands in random order, a short last band last
            in.listed = true;
            for (int b = 0; b < n_bands; ++b)
                if (rng() % 2) c.list.push_back(b);
            std::shuffle(c.list.begin(), c.list.end(), rng);
            if (in.height % in.band_rows != 0)
                for (size_t k = 0; k + 1 < c.list.size(); ++k)
                    if (c.list[k] == n_bands - 1) std::swap(c.list[k], c.list.back());
        } else {
            in.band_count = pick(1, 8);
            in.band_index = pick(0, in.band_count - 1);
        }
        in.spp = rng() % 3 ? pick(1, 64) : pick(64, 5000);
        in.flags = rng() % 8 == 0 ? TPT_FLAG_REF_ORDER : 0;
        in.lanes_per_pixel = pick(0, 2);
        in.spp_per_launch = rng() % 4 == 0 ? pick(1, in.spp) : 0;
        in.pipe_sets = pick(0, 5);
        in.pipe_chunks = rng() % 2 ? pick(1, 20) : 0;
        in.n_faces = rng() % 2 ? 1932 : 131072;
        in.n_lights = rng() % 3 == 0;
        in.n_materials = pick(0, 8);
        in.resident_lanes = (uint64_t)kRes[rng() % 3];
        in.env_is = rng() % 5 == 0;
        in.quad_fits = rng() % 4 != 0;
        c.finish();
    }
}

static int check_plan_sweep(int n, unsigned seed) {
    std::mt19937 rng(seed);
    int planned = 0;
    for (int i = 0; i < n; ++i) {
        PlanCase c;
        random_case(rng, c);
        const tpt::LaunchPlan pl = tpt::plan_launches(c.in);
        if (pl.status != TPT_OK) continue;
        ++planned;
        if (const char* what = plan_broken(c, pl)) {
            std::printf("error: case %d: %s\n", i, what);
            print_plan(c, pl);
            return 1;
        }
    }
    std::printf("ok plan sweep: %d of %d cases planned\n", planned, n);
    return 0;
}

static const char* const kFamilyName[tpt::kTraceFamilies] = {"lane", "drain", "pair", "is", "quad", "ref", "is_pair", "ref_is"};

static void print_key(const tpt::TraceKey& k, FILE* to) {
    const tpt::TraceFamilyInfo& f = tpt::kTraceFamily[k.family];
    std::fprintf(to, "\"family\":\"%s\",\"env_is\":%d,\"lanes\":%d,\"deep\":%d,\"lights\":%d,\"mtl_lds\":%d,\"wide_ids\":%d,"
                "\"noemit\":%d,\"legal\":%d,\"packed\":%u",
                kFamilyName[k.family], f.env_is, f.lanes, k.deep, k.lights, k.mtl_lds, k.wide_ids, k.noemit,
                tpt::trace_key_legal(k), tpt::trace_key_pack(k));
}

// "table": the family rows and the number of legal keys.  Else key=value,...:
//   select=1, ref env_is pair quad drained lights mtls faces depth emitter  (what launch_trace sees; default: box-like,
//             no lights, 5 materials, 1,932 faces, depth 8, an emitter)
//   layout=1, family (a name above) lights mtl_lds wide_ids wgw (0: the family's) stack depth mtls max_slots max_levels
static bool variant_case(const std::string& text, FILE* to = stdout) {
    if (text == "table") {
        std::fprintf(to, "{\"families\":[");
        for (int f = 0; f < tpt::kTraceFamilies; ++f) {
            const tpt::TraceFamilyInfo& r = tpt::kTraceFamily[f];
            std::fprintf(to, "%s[\"%s\",%d,%d,%d,%d,%d,%d,%d,%d]", f ? "," : "", kFamilyName[f], r.wgw, r.waves, r.lds_waves, r.lanes,
                        r.tile_w, r.tile_rows, r.env_is, r.ordered);
        }
        int legal = 0, round_trip = 0;
        for (unsigned p = 0; p < (1u << tpt::kTraceKeyBits); ++p) {
            legal += tpt::trace_key_legal(tpt::trace_key_unpack(p));
            round_trip += tpt::trace_key_pack(tpt::trace_key_unpack(p)) == p;
        }
        std::fprintf(to, "],\"public\":%d,\"legal_keys\":%d,\"round_trip\":%d}\n", tpt::kTracePublicFamilies, legal, round_trip);
        return true;
    }
    tpt::TraceSelectIn in{false, false, false, false, false, 0, 5, 1932, 8, true};
    tpt::TraceKey k{tpt::TF_LANE, false, false, false, false, false};
    long long mode = 0, wgw = 0, stack = 0, depth = 8, mtls = 5, max_slots = -1, max_levels = -1;
    size_t at = 0;
    while (at < text.size()) {
        const size_t end = std::min(text.find(',', at), text.size()), eq = text.find('=', at);
        if (eq == std::string::npos || eq >= end) return false;
        const std::string key = text.substr(at, eq - at), val = text.substr(eq + 1, end - eq - 1);
        const long long v = std::atoll(val.c_str());
        if (key == "select") mode = 1;
        else if (key == "layout") mode = 2;
        else if (key == "ref") in.ref_order = v != 0;
        else if (key == "env_is") in.env_is = v != 0;
        else if (key == "pair") in.pair = v != 0;
        else if (key == "quad") in.quad = v != 0;
        else if (key == "drained") in.drained = v != 0;
        else if (key == "emitter") in.any_emitter = v != 0;
        else if (key == "faces") in.n_faces = (int)v;
        else if (key == "depth") in.max_depth = (int)(depth = v);
        else if (key == "mtls") in.n_materials = (int)(mtls = v);
        else if (key == "lights") in.n_lights = (int)v, k.lights = v != 0;
        else if (key == "mtl_lds") k.mtl_lds = v != 0;
        else if (key == "wide_ids") k.wide_ids = v != 0;
        else if (key == "wgw") wgw = v;
        else if (key == "stack") stack = v;
        else if (key == "max_slots") max_slots = v;
        else if (key == "max_levels") max_levels = v;
        else if (key == "family") {
            int f = 0;
            while (f < tpt::kTraceFamilies && val != kFamilyName[f]) ++f;
            if (f == tpt::kTraceFamilies) return false;
            k.family = (tpt::TraceFamily)f;
        } else {
            return false;
        }
        at = end + 1;
    }
    if (mode == 1) {
        const tpt::TraceSelection s = tpt::select_trace_variant(in);
        if (s.error) {
            std::fprintf(to, "{\"error\":\"%s\"}\n", s.error);
            return true;
        }
        std::fprintf(to, "{");
        print_key(s.key, to);
        std::fprintf(to, "}\n");
        return true;
    }
    if (mode != 2) return false;
    const tpt::TraceLds l = tpt::trace_lds_layout(k, wgw > 0 ? (int)wgw : tpt::kTraceFamily[k.family].wgw, (int)stack, (int)depth,
                                                  (int)mtls, (size_t)max_slots, (size_t)max_levels);
    std::fprintf(to, "{\"bytes\":%zu,\"mtl_offset\":%d,\"stack_offset\":%d,\"rec_offset\":%d,\"stack_slots\":%d,\"rec_levels\":%d}\n",
                l.bytes, l.mtl_offset, l.stack_offset, l.rec_offset, l.stack_slots, l.rec_levels);
    return true;
}

// The planner and launch_trace agree: for every plan that succeeds, the variant the
// kernel side selects for the plan's requests runs two lanes per pixel exactly when
// the plan says so, and its tile has the plan's workgroup rows.
static int check_variant_sweep(int n, unsigned seed) {
    std::mt19937 rng(seed);
    int planned = 0, families[tpt::kTraceFamilies] = {};
    for (int i = 0; i < n; ++i) {
        PlanCase c;
        random_case(rng, c);
        tpt::PlanInput& in = c.in;
        static const int kMtls[] = {63, 64, 0x7ffd, 0x7ffe};
        static const int kFaces[] = {6, 32768, 32769};
        static const int kDepth[] = {1, 8, 9, 64};
        if (rng() % 4 == 0) in.n_materials = kMtls[rng() % 4];
        if (rng() % 4 == 0) in.n_faces = kFaces[rng() % 3];
        if (rng() % 4 == 0) in.lanes_per_pixel = 4;
        in.n_lights = in.n_lights ? 1 + (int)(rng() % 16) : 0;
        in.max_depth = kDepth[rng() % 4];
        in.any_emitter = rng() % 2 != 0;
        const tpt::LaunchPlan pl = tpt::plan_launches(in);
        if (pl.status != TPT_OK) continue;
        const tpt::TraceSelection s = tpt::select_trace_variant(
            {(in.flags & TPT_FLAG_REF_ORDER) != 0, in.env_is, pl.pair, pl.quad, pl.drained, in.n_lights, in.n_materials,
             in.n_faces, in.max_depth, in.any_emitter});
        // (quad_fits is the planner's word of trace_quad_fits, which refuses what the selection refuses)
        if (s.error && pl.quad && tpt::rec_words(in.n_lights, in.n_materials) == 5) continue;
        ++planned;
        const tpt::TraceFamilyInfo& f = tpt::kTraceFamily[s.key.family];
        ++families[s.key.family];
        if (s.error || !tpt::trace_key_legal(s.key) || pl.pair_kernel != (f.lanes == 2) || pl.wg_rows != f.tile_rows ||
            pl.quad != (f.lanes == 4)) {
            std::printf("error: case %d: plan pair_kernel %d quad %d wg_rows %d, selected %s (%d lanes, %d rows)%s%s\n", i,
                        pl.pair_kernel, pl.quad, pl.wg_rows, kFamilyName[s.key.family], f.lanes, f.tile_rows,
                        s.error ? ": " : "", s.error ? s.error : "");
            return 1;
        }
    }
    std::printf("ok variant sweep: %d of %d cases planned; families", planned, n);
    for (int f = 0; f < tpt::kTraceFamilies; ++f) std::printf(" %s=%d", kFamilyName[f], families[f]);
    std::printf("\n");
    return 0;
}

static int check_wide(int n, unsigned seed, int threads) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> u(-10.0f, 10.0f), e(0.0f, 2.0f);
    std::vector<float> box(6 * (size_t)n);
    std::vector<uint32_t> emit((size_t)n);
    for (int i = 0; i < n; ++i) {
        float c[3];
        for (int k = 0; k < 3; ++k) c[k] = (rng() % 7 == 0) ? 0.0f : u(rng);   // duplicated centroids
        for (int k = 0; k < 3; ++k) {
            const float h = (rng() % 5 == 0) ? 0.0f : e(rng);                // flat and point boxes
            box[6 * i + k] = c[k] - h;
            box[6 * i + 3 + k] = c[k] + h;
        }
        emit[i] = rng() % 11 == 0;
    }
    std::vector<int> pos((size_t)n);
    for (int i = 0; i < n; ++i) pos[i] = i;
    tpt::HostFloats out;
    int need = 0;
    tpt::WideParams prm;
    prm.threads = threads;
    const int nodes = tpt::build_wide_sah(pos, box.data(), emit.data(), n - 1, 0, out, &need, prm);
    if (nodes <= 0 || out.size() < 32 * (size_t)nodes || need <= 0) {
        std::printf("error: wide tree n=%d nodes=%d need=%d\n", n, nodes, need);
        return 1;
    }
    if (threads != 1) {   // the threaded build must equal the serial one byte for byte
        tpt::HostFloats ser;
        int sneed = 0;
        prm.threads = 1;
        const int snodes = tpt::build_wide_sah(pos, box.data(), emit.data(), n - 1, 0, ser, &sneed, prm);
        if (snodes != nodes || sneed != need || ser.size() != out.size() ||
            std::memcmp(ser.data(), out.data(), out.size() * sizeof(float)) != 0) {
            std::printf("error: wide tree n=%d threads=%d differs from the serial build\n", n, threads);
            return 1;
        }
    }
    {   // a reused workspace (the scene's, frame after frame) builds the same tree,
        // also after a build of another size in it
        tpt::WideWorkspace ws;
        tpt::WideParams wp;
        wp.threads = threads;
        wp.ws = &ws;
        std::vector<int> half(pos.begin(), pos.begin() + (n + 1) / 2);
        for (int rep = 0; rep < 3; ++rep) {
            tpt::HostFloats o2;
            int n2 = 0;
            const std::vector<int>& pp = rep == 1 ? half : pos;
            const int k = tpt::build_wide_sah(pp, box.data(), emit.data(), n - 1, 0, o2, &n2, wp);
            if (rep != 1 && (k != nodes || n2 != need || o2.size() != out.size() ||
                             std::memcmp(o2.data(), out.data(), out.size() * sizeof(float)) != 0)) {
                std::printf("error: wide tree n=%d: a reused workspace builds another tree\n", n);
                return 1;
            }
        }
    }
    std::printf("ok wide n=%d nodes=%d stack=%d\n", n, nodes, need);
    return 0;
}

// n threads, released together by one flag, each run work(thread); returns once all are joined.
template <class F>
static void run_together(int n, F work) {
    std::atomic<int> ready{0};
    std::atomic<bool> go{false};
    std::vector<std::thread> th;
    for (int i = 0; i < n; ++i)
        th.emplace_back([&, i] {
            ready.fetch_add(1);
            while (!go.load(std::memory_order_acquire)) {
            }
            work(i);
        });
    while (ready.load() < n) std::this_thread::yield();
    go.store(true, std::memory_order_release);
    for (std::thread& t : th) t.join();
}

// The process's first host_jumps() calls, made by n threads at once: what each thread sees at
// the moment the call returns must be the finished table.
static int check_jumps(int n) {
    const size_t words = (size_t)tpt::kRngJumps * tpt::kJumpWords;
    std::vector<uint32_t> ref(words);
    tpt::xorwow_jump_matrices(tpt::kRngJumps, ref.data());
    std::vector<std::vector<uint32_t>> seen((size_t)n);
    run_together(n, [&](int i) {
        const auto& j = tpt::host::host_jumps();
        seen[(size_t)i].assign(j.begin(), j.end());
    });
    int bad = 0;
    for (int i = 0; i < n; ++i) {
        const std::vector<uint32_t>& s = seen[(size_t)i];
        size_t wrong = 0, first = words;
        for (size_t k = 0; k < std::min(words, s.size()); ++k)
            if (s[k] != ref[k]) {
                ++wrong;
                first = std::min(first, k);
            }
        if (s.size() != words || wrong) {
            std::printf("differs %d: %zu of %zu words, %zu wrong, the first at %zu\n", i, s.size(), words, wrong, first);
            ++bad;
        }
    }
    if (bad) return 1;
    std::printf("ok jumps: %d threads saw the serial table (%zu words)\n", n, words);
    return 0;
}

// What one thread of parse-threads does, on objects of its own: every scene and image loaded,
// every plan and variant case run; the results as one string of bytes.  Throws what the loaders throw.
struct ParseWork {
    std::vector<std::string> gltf, image, plan, variant;
};
static std::string parse_work(const ParseWork& w) {
    std::string out;
    auto put = [&out](const void* p, size_t bytes) {
        const uint64_t n = bytes;
        out.append((const char*)&n, sizeof n);
        out.append((const char*)p, bytes);
    };
    for (const std::string& path : w.gltf) {
        tpt::HostScene hs;
        tpt::load_gltf(path, hs);
        put(hs.indices.data(), hs.indices.size() * sizeof(uint32_t));
        put(hs.vertices.data(), hs.vertices.size() * sizeof(float));
        put(hs.normals.data(), hs.normals.size() * sizeof(float));
        put(hs.lut.data(), hs.lut.size() * sizeof(tpt_interval));
        put(hs.vert_trans.data(), hs.vert_trans.size() * sizeof(float));
        put(hs.normal_trans.data(), hs.normal_trans.size() * sizeof(float));
        put(hs.materials.data(), hs.materials.size() * sizeof(tpt_material));
        put(hs.lights.data(), hs.lights.size() * sizeof(tpt_light));
        put(&hs.camera, sizeof hs.camera);
        out.push_back(hs.missing_material ? '1' : '0');
    }
    for (const std::string& path : w.image) {
        std::vector<uint8_t> rgba;
        int32_t wh[2] = {0, 0};
        tpt::load_image(path, rgba, wh[0], wh[1]);
        put(wh, sizeof wh);
        put(rgba.data(), rgba.size());
    }
    char* text = nullptr;
    size_t len = 0;
    FILE* f = open_memstream(&text, &len);
    if (!f) throw std::runtime_error("open_memstream failed");
    bool good = true;
    for (const std::string& c : w.plan) {
        PlanCase pc;
        good = good && plan_case(c, pc);
        if (good) print_plan(pc, tpt::plan_launches(pc.in), f);
    }
    for (const std::string& c : w.variant) good = good && variant_case(c, f);
    std::fclose(f);
    out.append(text, len);
    std::free(text);
    if (!good) throw std::runtime_error("bad plan or variant case");
    return out;
}

// parse-threads N [--gltf FILE...] [--image FILE...] [--plan CASE...] [--variant CASE...]: the loaders,
// the planner and the variant selection keep no state between calls, so n threads doing the same work at
// once each get the bytes the serial run got.
static int check_parse_threads(int n, int argc, char** argv) {
    ParseWork w;
    std::vector<std::string>* into = nullptr;
    for (int i = 0; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--gltf") into = &w.gltf;
        else if (a == "--image") into = &w.image;
        else if (a == "--plan") into = &w.plan;
        else if (a == "--variant") into = &w.variant;
        else if (into) into->push_back(a);
        else return 2;
    }
    std::string serial;
    try {
        serial = parse_work(w);
    } catch (const std::exception& ex) {
        std::printf("error: serial run: %s\n", ex.what());
        return 1;
    }
    std::vector<std::string> got((size_t)n), err((size_t)n);
    run_together(n, [&](int i) {
        const ParseWork mine = w;
        try {
            got[(size_t)i] = parse_work(mine);
        } catch (const std::exception& ex) {
            err[(size_t)i] = std::string("error: ") + ex.what();
        }
    });
    int bad = 0;
    for (int i = 0; i < n; ++i) {
        if (err[(size_t)i].empty() && got[(size_t)i] == serial) continue;
        size_t k = 0;
        while (k < std::min(serial.size(), got[(size_t)i].size()) && serial[k] == got[(size_t)i][k]) ++k;
        std::printf("differs %d: %zu bytes against %zu, the first at %zu %s\n", i, got[(size_t)i].size(), serial.size(), k,
                    err[(size_t)i].c_str());
        ++bad;
    }
    if (bad) return 1;
    std::printf("ok parse-threads: %d threads, %zu scenes, %zu images, %zu plans, %zu variant cases, %zu bytes each\n", n,
                w.gltf.size(), w.image.size(), w.plan.size(), w.variant.size(), serial.size());
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: host_check gltf|image FILE... | wide N SEED [THREADS] | plan CASE... | "
                             "plan-sweep N SEED | variant CASE... | variant-sweep N SEED | jumps N | "
                             "parse-threads N [--gltf FILE...] [--image FILE...] [--plan CASE...] [--variant CASE...]\n");
        return 2;
    }
    const std::string mode = argv[1];
    if (mode == "jumps") return check_jumps(std::max(std::atoi(argv[2]), 1));
    if (mode == "parse-threads") return check_parse_threads(std::max(std::atoi(argv[2]), 1), argc - 3, argv + 3);
    if (mode == "plan-sweep") return check_plan_sweep(std::atoi(argv[2]), argc > 3 ? (unsigned)std::atoi(argv[3]) : 1u);
    if (mode == "variant-sweep")
        return check_variant_sweep(std::atoi(argv[2]), argc > 3 ? (unsigned)std::atoi(argv[3]) : 1u);
    if (mode == "variant") {
        for (int i = 2; i < argc; ++i)
            if (!variant_case(argv[i])) {
                std::printf("error: bad case %s\n", argv[i]);
                return 1;
            }
        return 0;
    }
    if (mode == "plan") {
        for (int i = 2; i < argc; ++i) {
            PlanCase c;
            if (!plan_case(argv[i], c)) {
                std::printf("error: bad case %s\n", argv[i]);
                return 1;
            }
            print_plan(c, tpt::plan_launches(c.in));
        }
        return 0;
    }
    if (mode == "wide")
        return check_wide(std::atoi(argv[2]), argc > 3 ? (unsigned)std::atoi(argv[3]) : 1u, argc > 4 ? std::atoi(argv[4]) : -1);
    for (int i = 2; i < argc; ++i) {
        try {
            if (mode == "gltf") {
                tpt::HostScene hs;
                tpt::load_gltf(argv[i], hs);
                std::printf("ok %zu faces\n", hs.indices.size() / 3);
            } else if (mode == "image") {
                std::vector<uint8_t> rgba;
                int w = 0, h = 0;
                tpt::load_image(argv[i], rgba, w, h);
                if (rgba.size() != 4 * (size_t)w * (size_t)h) {
                    std::printf("error: size mismatch\n");
                    return 1;
                }
                std::printf("ok %dx%d\n", w, h);
            } else {
                return 2;
            }
        } catch (const std::exception& ex) {
            std::printf("error: %s\n", ex.what());
        }
    }
    return 0;
}
