// plan_tiles_check CASE...: plan_launches (host/launch_plan.cpp) on listed launches, the launches
// of tpt_render_adaptive over a list of 16x16-pixel tiles (PlanInput::n_tiles).  CPU only, built by
// tests/test_adaptive_plan_cpu.py with the host compiler (under ASan + UBSan where it has them).
//
// CASE is key=value,...: w h bh (rows this call renders; default h) bc bi frames listed | spp flags
// lanes sets chunks spl | faces lights resident env_is quad_fits | tiles (default -1: an unlisted
// launch).  Defaults as tests/sanitize/host_check.cpp "plan": 327,680 resident lanes, quad_fits.
// One JSON line per case.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "launch_plan.hpp"

static bool parse(const std::string& text, tpt::PlanInput& in) {
    in.resident_lanes = 327680;
    in.quad_fits = true;
    long long bh = -1;
    size_t at = 0;
    while (at < text.size()) {
        size_t end = text.find(',', at);
        if (end == std::string::npos) end = text.size();
        const size_t eq = text.find('=', at);
        if (eq == std::string::npos || eq >= end) return false;
        const std::string key = text.substr(at, eq - at);
        const long long v = std::atoll(text.substr(eq + 1, end - eq - 1).c_str());
        if (key == "w") in.width = (int32_t)v;
        else if (key == "h") in.height = (int32_t)v;
        else if (key == "bh") bh = v;
        else if (key == "bc") in.band_count = (int32_t)v;
        else if (key == "bi") in.band_index = (int32_t)v;
        else if (key == "frames") in.n_frames = (int32_t)v;
        else if (key == "listed") in.listed = v != 0;
        else if (key == "spp") in.spp = (int32_t)v;
        else if (key == "flags") in.flags = (int32_t)v;
        else if (key == "lanes") in.lanes_per_pixel = (int32_t)v;
        else if (key == "sets") in.pipe_sets = (int32_t)v;
        else if (key == "chunks") in.pipe_chunks = (int32_t)v;
        else if (key == "spl") in.spp_per_launch = (int32_t)v;
        else if (key == "faces") in.n_faces = (int32_t)v;
        else if (key == "lights") in.n_lights = (int32_t)v;
        else if (key == "resident") in.resident_lanes = (uint64_t)v;
        else if (key == "env_is") in.env_is = v != 0;
        else if (key == "quad_fits") in.quad_fits = v != 0;
        else if (key == "tiles") in.n_tiles = (int32_t)v;
        else return false;
        at = end + 1;
    }
    in.bh = bh >= 0 ? (int32_t)bh : in.height;
    return true;
}

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) {
        tpt::PlanInput in;
        if (!parse(argv[i], in)) {
            std::printf("error: bad case %s\n", argv[i]);
            return 1;
        }
        const tpt::LaunchPlan pl = tpt::plan_launches(in);
        if (pl.status != TPT_OK) {
            std::printf("{\"status\":%d,\"message\":\"%s\"}\n", (int)pl.status, pl.message);
            continue;
        }
        std::printf("{\"status\":0,\"pair\":%d,\"pair_kernel\":%d,\"quad\":%d,\"drained\":%d,\"refill\":%d,"
                    "\"leaf_kb\":%d,\"xcd_run\":%d,\"nset\":%d,\"chunk\":%d,\"launches\":[",
                    pl.pair, pl.pair_kernel, pl.quad, pl.drained, pl.refill, pl.leaf_kb, pl.xcd_run, pl.nset, pl.chunk);
        for (size_t j = 0; j < pl.order.size(); ++j)
            std::printf(j ? ",[%d,%d]" : "[%d,%d]", pl.launches[pl.order[j]].set, pl.launches[pl.order[j]].samples);
        std::printf("]}\n");
    }
    return 0;
}
