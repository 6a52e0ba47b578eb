// tpt_render -- headless replacement for the reference's main.cu + Vulkan
// display loop (src/main.cu:6-14, src/vkEngine.cu:180-302): renders one glTF
// scene through the C++ host API (tpt.hpp) and writes the framebuffer as PPM
// (8-bit, copyToFB's truncating tone map) and the radiance as PFM (fp32).
//
//   tpt_render scene.gltf [--width W] [--height H] [--spp N] [--depth D]
//              [--seed S] [--env equirect.jpg|.ppm|--sky] [--out prefix] [--device i]
//              [--frames F [--progressive]] [--aov] [--denoise [iterations]]
//              [--temporal] [--yaw DEG] [--svgf [iterations]] [--aov-path [bounces]]
//              [--move OBJ DX DY DZ] [--spin OBJ DEG] [--wave OBJ AMP] [--refit]
//              [--adaptive TARGET [--min-spp N] [--max-spp N]]
//              [--clip [GAMMA]] [--clip-radius R] [--clip-history N] [--scale S]
//              [--tonemap [linear|reinhard|aces]] [--ev STOPS] [--auto-exposure [KEY]] [--adapt RATE]
//              [--srgb | --gamma G] [--dither]
// --aov writes the first-hit feature buffers <out>_albedo.pfm, <out>_normal.pfm and
// <out>_depth.pfm (tpt_render_aov); --denoise writes <out>_denoised.pfm / .ppm, the
// a-trous filter of the written frame (tpt_denoise, the hosts' defaults; with
// --progressive the written frame is the accumulated one).  --temporal runs every
// frame (frame i with seed S + i) and its feature buffers through tpt_temporal and
// writes <out>_temporal.pfm / .ppm for the last one; --denoise then filters that.
// --svgf writes <out>_svgf.pfm / .ppm, the variance-guided filter (tpt_denoise_svgf, the
// hosts' defaults): with --temporal of the accumulated frame, by that pass's variance
// and history length; without it of the written frame, on the spatial variance
// estimate alone.  --denoise and --svgf may be combined: both files are written.
// --aov-path follows perfect mirrors (tpt_render_aov_path, up to `bounces` of them, default 8):
// <out>_albedo.pfm, <out>_normal.pfm and <out>_depth.pfm are written from the path buffers,
// with <out>_bounces.pfm, and --denoise / --svgf take them as guides; --temporal keeps the
// first-hit buffers, whose surface it reprojects.
// --adaptive TARGET renders every 16x16-pixel tile until its error estimate is below TARGET
// (tpt_render_adaptive), from --min-spp (default 16) to at most --max-spp (default 1024, min-spp
// times a power of two) samples; --spp is not used.  <out>_spp.pfm holds every pixel's sample
// count.  --aov, --aov-path, --denoise and --svgf run on its frame as on a fixed-spp one; not with
// --temporal, --progressive, --frames, --yaw or --truck (one frame from the scene's camera), and
// --min-spp / --max-spp are refused without it.
// --yaw DEG turns the camera about its own origin and up axis by DEG per frame.
// --move OBJ DX DY DZ translates object OBJ (its index in the scene's object order: the
// mesh nodes of the glTF file in node order) by (DX, DY, DZ) world units per frame; --spin
// OBJ DEG turns it by DEG per frame about world +y through the centre of its frame-0 world
// bounding box (with both, it turns first).  Either needs --frames and --temporal: every
// frame sets the transforms (tpt_scene_set_transforms), rebuilds, renders, and goes
// through tpt_temporal_motion, which follows the moved objects.
// --wave OBJ AMP displaces every vertex of object OBJ along its own object-space normal by
// AMP sin(6 y_obj + frame) in frame `frame` (a deformation no matrix describes), under the same
// conditions as --move: every frame sets the vertices (tpt_scene_set_vertices), rebuilds, renders,
// and goes through tpt_temporal_deform, which follows the deformed mesh (and --move / --spin too).
// --clip [GAMMA] (with --temporal or --temporal-path) turns history clipping on
// (tpt_history_set_clip, the hosts' defaults): the reprojected history is clamped to mean +- GAMMA
// standard deviations of the frame's colours around each pixel, so that a moved object's shadow
// and its reflections stop lagging; --clip-radius R (1..3) and --clip-history N set the window and
// the cap on a clipped pixel's history length.  Each frame prints its reprojected and clipped
// pixel counts on stderr.
// --scale S (2..4) traces every frame at ceil(W / S) x ceil(H / S) and makes the W x H frame of it
// by guided upsampling (tpt_upsample, the hosts' defaults) on the feature buffers of both sizes:
// everything after it -- --temporal*, --clip, --denoise, --svgf, the .pfm / .ppm outputs -- sees the
// full-size frame.  <out>_low.pfm holds the traced frame, and each frame prints its fallback pixel
// count on stderr.  With --aov-path both guide sets are the path buffers and the colours are
// demodulated.  Not with --adaptive or --progressive.
// --tonemap [linear|reinhard|aces] (default reinhard) writes <out>_display.ppm, the display stage
// (tpt_tonemap, the hosts' defaults but no transfer function unless --srgb or --gamma G is given) of
// the last frame the chain produced: the render (upsampled under --scale), or the output of
// --temporal*, --denoise or --svgf (of --svgf where both are given).  --ev STOPS is the fixed
// exposure (added to the measured one under --auto-exposure); --auto-exposure [KEY] measures each
// frame's exposure (key 0.18 unless given); --adapt RATE moves the exposure that far towards each
// frame's target; --dither adds the ordered dither.  With --frames F and --temporal* every frame's
// accumulated output goes through one tpt_exposure and prints its scale on stderr; the file holds
// the last frame, and a --denoise / --svgf output is mapped at the scale that frame got.  Every
// other file is written as without these options; all of them but --tonemap are refused without it.
// --refit (with --move / --spin / --wave): the frames after the first refit the BVH
// (tpt_scene_refit) instead of rebuilding it, and each prints its tree cost against the built
// one and the refit's device time on stderr.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "tpt.hpp"

namespace {

// Deterministic procedural sky (stand-in for the missing kloppenheim_07 env,
// SURVEY 8(d) C3); same formula as tinypathtracer_amd.procedural_sky.
std::vector<uint8_t> procedural_sky(int w, int h) {
    std::vector<uint8_t> img((size_t)w * h * 4);
    for (int y = 0; y < h; ++y) {
        const double theta = (y + 0.5) / h * M_PI;
        const double elev = std::cos(theta);
        const double sky = elev > 0 ? elev : 0.0, ground = elev < 0 ? -elev : 0.0;
        for (int x = 0; x < w; ++x) {
            const double phi = (x + 0.5) / w * 2.0 * M_PI;
            const double sun = std::exp(-((theta - 0.9) * (theta - 0.9) + (std::cos(phi) - 1.0) * (std::cos(phi) - 1.0)) * 40.0);
            const double c[3] = {0.45 + 0.25 * sky - 0.25 * ground + 0.5 * sun,
                                 0.55 + 0.25 * sky - 0.30 * ground + 0.45 * sun,
                                 0.75 + 0.20 * sky - 0.45 * ground + 0.30 * sun};
            for (int k = 0; k < 3; ++k) {
                double v = c[k] * 255.0;
                v = v < 0 ? 0 : (v > 255 ? 255 : v);
                img[((size_t)y * w + x) * 4 + k] = (uint8_t)v;
            }
            img[((size_t)y * w + x) * 4 + 3] = 255;
        }
    }
    return img;
}

void write_ppm(const std::string& path, const std::vector<uint8_t>& bgra, int W, int H) {
    std::ofstream ppm(path, std::ios::binary);
    ppm << "P6\n" << W << " " << H << "\n255\n";
    for (size_t i = 0; i < (size_t)W * H; ++i) {   // BGRA -> RGB, rows already top-down
        const char px[3] = {(char)bgra[4 * i + 2], (char)bgra[4 * i + 1], (char)bgra[4 * i]};
        ppm.write(px, 3);
    }
}

// PFM rows are bottom-up, like the radiance and the feature buffers; 3 channels "PF", 1 channel "Pf"
void write_pfm(const std::string& path, const std::vector<float>& v, int W, int H, int channels) {
    std::ofstream pfm(path, std::ios::binary);
    pfm << (channels == 3 ? "PF" : "Pf") << "\n" << W << " " << H << "\n-1.0\n";
    pfm.write((const char*)v.data(), (std::streamsize)(v.size() * sizeof(float)));
}

const char* kUsage =
    "usage: %s scene.gltf [--width W] [--height H] [--spp N] [--depth D] [--seed S] "
    "[--env file.jpg|file.ppm | --sky] [--out prefix] [--device i] [--frames F [--progressive]] "
    "[--aov] [--denoise [iterations]] [--temporal] [--yaw DEG] [--svgf [iterations]] "
    "[--aov-path [bounces]] [--move OBJ DX DY DZ] [--spin OBJ DEG] [--wave OBJ AMP] [--refit] [--truck DX DY DZ] "
    "[--temporal-path [bounces]] [--adaptive TARGET [--min-spp N] [--max-spp N]] "
    "[--clip [GAMMA]] [--clip-radius R] [--clip-history N] [--scale S] "
    "[--tonemap [linear|reinhard|aces]] [--ev STOPS] [--auto-exposure [KEY]] [--adapt RATE] "
    "[--srgb | --gamma G] [--dither]\n";

// The scene's camera turned by `deg` degrees about its own origin and up axis: c2w * R_y
tpt::Camera yawed(const tpt::Camera& base, double deg) {
    tpt::Camera cam = base;
    const double t = deg * M_PI / 180.0, c = std::cos(t), s = std::sin(t);
    for (int i = 0; i < 4; ++i) {
        const double right = base.c.c2w[i], back = base.c.c2w[8 + i];
        cam.c.c2w[i] = (float)(c * right - s * back);
        cam.c.c2w[8 + i] = (float)(s * right + c * back);
    }
    return cam;
}

// `base` with its origin shifted by `shift` in world space (--truck, per frame)
tpt::Camera trucked(const tpt::Camera& base, const double* shift, int frame) {
    tpt::Camera cam = base;
    for (int r = 0; r < 3; ++r) cam.c.c2w[12 + r] = base.c.c2w[12 + r] + (float)(shift[r] * frame);
    return cam;
}

// --move / --spin: what one object does per frame
struct ObjectMotion {
    uint32_t object = 0;
    double move[3] = {0.0, 0.0, 0.0};
    double spin = 0.0;          // degrees about world +y
    double centre[3] = {0.0, 0.0, 0.0};   // of the frame-0 world bounding box
};

// The centre of object o's world bounding box under its matrix in the desc
void world_box_centre(const tpt_scene_desc& d, uint32_t o, double* centre) {
    const uint32_t begin = (uint32_t)d.lut[o].begin, end = o + 1 < d.n_objects ? (uint32_t)d.lut[o + 1].begin : d.n_faces;
    const float* m = d.vert_trans + 16 * (size_t)o;
    double lo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, hi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    for (uint32_t i = 3 * begin; i < 3 * end; ++i) {
        const float* v = d.vertices + 3 * (size_t)d.indices[i];
        for (int r = 0; r < 3; ++r) {
            const double w = (double)m[r] * v[0] + (double)m[4 + r] * v[1] + (double)m[8 + r] * v[2] + (double)m[12 + r];
            lo[r] = std::min(lo[r], w);
            hi[r] = std::max(hi[r], w);
        }
    }
    for (int r = 0; r < 3; ++r) centre[r] = 0.5 * (lo[r] + hi[r]);
}

// Frame `frame`'s matrix of a moving object: T(frame * move) T(c) R_y(frame * spin) T(-c) M0,
// in double, rounded to float once; frame 0 is M0 itself
void moved_matrix(const ObjectMotion& om, const float* m0, int frame, float* out) {
    if (frame == 0) {
        std::memcpy(out, m0, 16 * sizeof(float));
        return;
    }
    const double t = om.spin * frame * M_PI / 180.0, c = std::cos(t), s = std::sin(t);
    const double rot[3][3] = {{c, 0.0, s}, {0.0, 1.0, 0.0}, {-s, 0.0, c}};
    for (int col = 0; col < 4; ++col) {
        double v[3] = {m0[4 * col], m0[4 * col + 1], m0[4 * col + 2]};
        if (col == 3)
            for (int r = 0; r < 3; ++r) v[r] -= om.centre[r];
        for (int r = 0; r < 3; ++r) {
            double w = rot[r][0] * v[0] + rot[r][1] * v[1] + rot[r][2] * v[2];
            if (col == 3) w += om.centre[r] + om.move[r] * frame;
            out[4 * col + r] = (float)w;
        }
        out[4 * col + 3] = m0[4 * col + 3];
    }
}

// --wave: object `object`'s vertices are the ids [first, first + rest.size() / 3) (those of
// that range its faces do not name keep their place)
struct ObjectWave {
    uint32_t object = 0;
    double amp = 0.0;
    uint32_t first = 0;
    std::vector<float> rest;        // the loaded positions of the range
    std::vector<uint8_t> mine;      // per vertex of the range: named by a face of the object
};

void wave_range(const tpt_scene_desc& d, ObjectWave& ow) {
    const uint32_t begin = (uint32_t)d.lut[ow.object].begin,
                   end = ow.object + 1 < d.n_objects ? (uint32_t)d.lut[ow.object + 1].begin : d.n_faces;
    uint32_t lo = d.n_vertices, hi = 0;
    for (uint32_t i = 3 * begin; i < 3 * end; ++i) {
        lo = std::min(lo, d.indices[i]);
        hi = std::max(hi, d.indices[i]);
    }
    if (lo > hi) throw std::runtime_error("--wave: the object has no faces");
    ow.first = lo;
    ow.rest.assign(d.vertices + 3 * (size_t)lo, d.vertices + 3 * ((size_t)hi + 1));
    ow.mine.assign((size_t)hi - lo + 1, 0);
    for (uint32_t i = 3 * begin; i < 3 * end; ++i) ow.mine[d.indices[i] - lo] = 1;
}

// Frame `frame`'s positions of the range: rest + AMP sin(6 y + frame) n, in float; frame 0 is
// displaced too (sin(6 y) is not 0), so every frame of a run is one pose of the same wave
void waved_vertices(const tpt_scene_desc& d, const ObjectWave& ow, int frame, std::vector<float>& out) {
    out = ow.rest;
    for (size_t k = 0; k < ow.mine.size(); ++k) {
        if (!ow.mine[k]) continue;
        const float* n = d.normals + 3 * ((size_t)ow.first + k);
        const float s = (float)(ow.amp * std::sin(6.0 * (double)ow.rest[3 * k + 1] + (double)frame));
        for (int r = 0; r < 3; ++r) out[3 * k + r] = ow.rest[3 * k + r] + s * n[r];
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, kUsage, argv[0]);
        return 2;
    }
    std::string scene_file = argv[1], env_file, out = "out";
    int W = 1920, H = 1080, spp = 64, depth = 8, device = 0, frames = 1;
    bool progressive = false, aov = false, denoise = false, temporal = false, svgf = false, aov_path = false;
    int path_bounces = 8;
    bool adaptive = false;               // --adaptive: tiles rendered to a target error
    float ad_target = 0.0f;
    int ad_min = 16, ad_max = 1024;
    bool ad_range = false;               // --min-spp or --max-spp given
    tpt_adaptive_stats ad_stats{};
    double yaw = 0.0;
    double truck[3] = {0.0, 0.0, 0.0};   // --truck: the camera's world-space shift per frame
    bool temporal_path = false;          // --temporal-path: accumulate on mirror-path guides
    std::vector<ObjectMotion> motions;   // --move / --spin, one entry per object named
    std::vector<ObjectWave> waves;       // --wave, one entry per option
    bool refit = false;                  // --refit: frames after the first refit instead of rebuilding
    bool clip = false, clip_opts = false;   // --clip; --clip-radius or --clip-history given
    tpt_clip_params clip_params = tpt::defaultClip();
    int scale = 1;                       // --scale: frames are traced at 1 / scale of the size and upsampled
    bool tonemap = false;                // --tonemap: <out>_display.ppm
    const char* tm_opt = nullptr;        // the first of --ev, --auto-exposure, --adapt, --srgb, --gamma, --dither given
    bool tm_adapt = false, tm_srgb = false, tm_gamma = false;
    tpt_tonemap_params tm = tpt::defaultTonemap();
    tm.transfer = TPT_TRANSFER_NONE;
    auto motion_of = [&](uint32_t object) -> ObjectMotion& {
        for (auto& om : motions)
            if (om.object == object) return om;
        motions.emplace_back();
        motions.back().object = object;
        return motions.back();
    };
    int dn_iterations = tpt::defaultDenoise().iterations;
    int sv_iterations = tpt::defaultSVGF().iterations;
    uint64_t seed = 0;
    bool sky = false;
    for (int i = 2; i < argc; ++i) {
        std::string a = argv[i];
        auto next = [&]() -> std::string {
            if (i + 1 >= argc) throw std::runtime_error("missing value for " + a);
            return argv[++i];
        };
        if (a == "--width") W = std::stoi(next());
        else if (a == "--height") H = std::stoi(next());
        else if (a == "--spp") spp = std::stoi(next());
        else if (a == "--depth") depth = std::stoi(next());
        else if (a == "--seed") seed = std::stoull(next());
        else if (a == "--env") env_file = next();
        else if (a == "--sky") sky = true;
        else if (a == "--out") out = next();
        else if (a == "--device") device = std::stoi(next());
        else if (a == "--frames") frames = std::stoi(next());
        else if (a == "--progressive") progressive = true;
        else if (a == "--aov") aov = true;
        else if (a == "--temporal") temporal = true;
        else if (a == "--aov-path") {
            aov_path = true;   // an optional bounce cap follows
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') path_bounces = std::stoi(argv[++i]);
        }
        else if (a == "--temporal-path") {
            temporal = temporal_path = true;   // an optional bounce cap follows
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') path_bounces = std::stoi(argv[++i]);
        }
        else if (a == "--adaptive") { adaptive = true; ad_target = std::stof(next()); }
        else if (a == "--min-spp") { ad_range = true; ad_min = std::stoi(next()); }
        else if (a == "--max-spp") { ad_range = true; ad_max = std::stoi(next()); }
        else if (a == "--yaw") yaw = std::stod(next());
        else if (a == "--truck") {
            for (double& v : truck) v = std::stod(next());
        }
        else if (a == "--move") {
            ObjectMotion& om = motion_of((uint32_t)std::stoul(next()));
            for (double& v : om.move) v = std::stod(next());
        }
        else if (a == "--spin") {
            ObjectMotion& om = motion_of((uint32_t)std::stoul(next()));
            om.spin = std::stod(next());
        }
        else if (a == "--wave") {
            waves.emplace_back();
            waves.back().object = (uint32_t)std::stoul(next());
            waves.back().amp = std::stod(next());
        }
        else if (a == "--refit") refit = true;
        else if (a == "--scale") {
            scale = std::stoi(next());
            if (scale < 2 || scale > 4) {
                std::fprintf(stderr, "--scale S: S must be 2..4\n");
                return 2;
            }
        }
        else if (a == "--tonemap") {
            tonemap = true;   // an optional operator follows
            if (i + 1 < argc && argv[i + 1][0] != '-') {
                const std::string op = argv[++i];
                if (op == "linear") tm.op = TPT_TONEMAP_LINEAR;
                else if (op == "reinhard") tm.op = TPT_TONEMAP_REINHARD;
                else if (op == "aces") tm.op = TPT_TONEMAP_ACES;
                else {
                    std::fprintf(stderr, "--tonemap: the operator must be linear, reinhard or aces\n");
                    return 2;
                }
            }
        }
        else if (a == "--ev") { tm_opt = tm_opt ? tm_opt : "--ev"; tm.ev = std::stof(next()); }
        else if (a == "--auto-exposure") {
            tm_opt = tm_opt ? tm_opt : "--auto-exposure";
            tm.flags |= TPT_TONEMAP_AUTO;   // an optional key follows
            if (i + 1 < argc && ((argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') || argv[i + 1][0] == '.'))
                tm.key = std::stof(argv[++i]);
        }
        else if (a == "--adapt") { tm_opt = tm_opt ? tm_opt : "--adapt"; tm_adapt = true; tm.rate = std::stof(next()); }
        else if (a == "--srgb") { tm_opt = tm_opt ? tm_opt : "--srgb"; tm_srgb = true; tm.transfer = TPT_TRANSFER_SRGB; }
        else if (a == "--gamma") {
            tm_opt = tm_opt ? tm_opt : "--gamma";
            tm_gamma = true;
            tm.transfer = TPT_TRANSFER_GAMMA;
            tm.gamma = std::stof(next());
        }
        else if (a == "--dither") { tm_opt = tm_opt ? tm_opt : "--dither"; tm.flags |= TPT_TONEMAP_DITHER; }
        else if (a == "--clip") {
            clip = true;   // an optional gamma follows
            if (i + 1 < argc && ((argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') || argv[i + 1][0] == '.'))
                clip_params.gamma = std::stof(argv[++i]);
        }
        else if (a == "--clip-radius") { clip = clip_opts = true; clip_params.radius = std::stoi(next()); }
        else if (a == "--clip-history") { clip = clip_opts = true; clip_params.max_history = std::stoi(next()); }
        else if (a == "--denoise") {
            denoise = true;   // an optional iteration count follows
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') dn_iterations = std::stoi(argv[++i]);
        }
        else if (a == "--svgf") {
            svgf = true;   // an optional iteration count follows
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') sv_iterations = std::stoi(argv[++i]);
        }
        else { std::fprintf(stderr, "unknown option %s\n", a.c_str()); return 2; }
    }
    if (!motions.empty() && progressive) {   // the accumulated samples belong to the scene as it was
        std::fprintf(stderr, "--move and --spin cannot be combined with --progressive\n");
        return 2;
    }
    if (!motions.empty() && (!temporal || frames < 2)) {
        std::fprintf(stderr, "--move and --spin need --frames F (F > 1) and --temporal\n");
        return 2;
    }
    if (!motions.empty() && temporal_path) {   // tpt_temporal_path does not follow moving objects
        std::fprintf(stderr, "--move and --spin cannot be combined with --temporal-path\n");
        return 2;
    }
    if (!waves.empty() && progressive) {   // as --move
        std::fprintf(stderr, "--wave cannot be combined with --progressive\n");
        return 2;
    }
    if (!waves.empty() && (!temporal || frames < 2)) {
        std::fprintf(stderr, "--wave needs --frames F (F > 1) and --temporal\n");
        return 2;
    }
    if (!waves.empty() && temporal_path) {   // tpt_temporal_path does not follow deforming meshes
        std::fprintf(stderr, "--wave cannot be combined with --temporal-path\n");
        return 2;
    }
    if (refit && motions.empty() && waves.empty()) {   // nothing moves: nothing to refit
        std::fprintf(stderr, "--refit needs --move, --spin or --wave\n");
        return 2;
    }
    if (clip && !temporal) {
        std::fprintf(stderr, "--clip, --clip-radius and --clip-history need --temporal or --temporal-path\n");
        return 2;
    }
    if (temporal && progressive) {   // progressive is already the exact accumulation of an unmoving camera
        std::fprintf(stderr, "--temporal cannot be combined with --progressive\n");
        return 2;
    }
    const bool camera_moves = yaw != 0.0 || truck[0] != 0.0 || truck[1] != 0.0 || truck[2] != 0.0;
    if (adaptive && (temporal || progressive || frames != 1 || camera_moves)) {
        std::fprintf(stderr, "--adaptive renders one frame: not with --temporal, --progressive, --frames, --yaw "
                             "or --truck\n");
        return 2;
    }
    if (scale > 1 && (adaptive || progressive)) {   // both accumulate samples in a full-size frame
        std::fprintf(stderr, "--scale cannot be combined with --adaptive or --progressive\n");
        return 2;
    }
    if (ad_range && !adaptive) {
        std::fprintf(stderr, "--min-spp and --max-spp need --adaptive TARGET\n");
        return 2;
    }
    if (tm_opt && !tonemap) {
        std::fprintf(stderr, "%s needs --tonemap\n", tm_opt);
        return 2;
    }
    if (tm_srgb && tm_gamma) {
        std::fprintf(stderr, "--srgb cannot be combined with --gamma\n");
        return 2;
    }
    if (tm_adapt && !(tm.flags & TPT_TONEMAP_AUTO)) {
        std::fprintf(stderr, "--adapt needs --auto-exposure\n");
        return 2;
    }
    if (!(tm.rate > 0.0f && tm.rate <= 1.0f)) {
        std::fprintf(stderr, "--adapt RATE: RATE must be in (0, 1]\n");
        return 2;
    }
    if (!(tm.gamma > 0.0f) || !(tm.key > 0.0f)) {
        std::fprintf(stderr, "--gamma G and --auto-exposure KEY: the value must be > 0\n");
        return 2;
    }
    try {
        tpt::EnvLight env;
        if (!env_file.empty()) {
            env = tpt::EnvLight(env_file, device);   // JPEG / PPM, decoded natively (tpt_env_load)
        } else if (sky) {
            auto img = procedural_sky(2048, 1024);
            env = tpt::EnvLight(img.data(), 2048, 1024, device);
        }
        tpt::PathTracer pt(env, W, H, device);
        // render(meshFile) (path_tracer.cu:556-579) spelled out, so the scene is still there for the post-pass
        tpt::Scene scene(scene_file, "gltf");
        tpt::DeviceScene d = scene.copySceneToDevice(device);
        d.build();
        for (auto& om : motions) {
            if (om.object >= scene.desc().n_objects) throw std::runtime_error("--move / --spin: no such object");
            world_box_centre(scene.desc(), om.object, om.centre);
        }
        for (auto& ow : waves) {
            if (ow.object >= scene.desc().n_objects) throw std::runtime_error("--wave: no such object");
            wave_range(scene.desc(), ow);
        }
        tpt::Frame f;
        f.width = W;
        f.height = H;
        f.bgra.assign((size_t)W * H * 4, 255);
        f.radiance.assign((size_t)W * H * 3, 0.0f);
        tpt::Camera cam = scene.m_camera;
        // One frame into f: traced at the full size, or (--scale) at the low size and upsampled by
        // the feature buffers of both sizes, so that everything after it sees a W x H frame
        const tpt::Size lo = tpt::lowSize(W, H, scale);
        tpt::PathTracer ptl(env, lo.width, lo.height, device);
        std::vector<float> low_rad;
        std::vector<uint8_t> low_bgra;
        auto trace = [&](const tpt::Camera& c, uint64_t sd, bool accumulate) {
            if (scale == 1) {
                f.stats = pt.doTrace(d, c, f.bgra.data(), spp, sd, depth, f.radiance.data(), 1, 0, accumulate);
                return;
            }
            low_rad.resize((size_t)lo.width * lo.height * 3);
            low_bgra.assign((size_t)lo.width * lo.height * 4, 255);
            f.stats = ptl.doTrace(d, c, low_bgra.data(), spp, sd, depth, low_rad.data());
            tpt::AOV gl = aov_path ? ptl.renderAOVPath(d, c, path_bounces) : ptl.renderAOV(d, c);
            tpt::AOV gf = aov_path ? pt.renderAOVPath(d, c, path_bounces) : pt.renderAOV(d, c);
            tpt_upsample_params up = tpt::defaultUpsample();
            if (aov_path) up.flags |= TPT_UPSAMPLE_DEMODULATE;
            const tpt_upsample_stats us = pt.upsample(d, lo.width, lo.height, low_rad.data(), gl.view(), gf.view(),
                                                      f.radiance.data(), f.bgra.data(), up);
            std::fprintf(stderr, "upsampled %d x %d to %d x %d: %llu fallback pixels, %.3f ms\n", lo.width, lo.height, W,
                         H, (unsigned long long)us.fallback, us.kernel_ms);
        };
        std::vector<float> acc;       // --temporal: the accumulated frame,
        std::vector<float> var, len;  //   its luminance variance and history length
        tpt::AOV g;
        // --tonemap: <out>_display.ppm from `rad`; the exposure lives as long as the frames do
        std::vector<uint8_t> display;
        std::unique_ptr<tpt::Exposure> exposure(tonemap ? new tpt::Exposure(d) : nullptr);
        tpt_tonemap_stats tms{};
        auto show = [&](const float* rad, const tpt_tonemap_params& prm) {
            display.assign((size_t)W * H * 4, 255);
            tms = pt.tonemap(d, rad, nullptr, display.data(), prm, exposure.get());
        };
        if (temporal) {
            tpt::History hist(d, W, H);
            if (clip) hist.setClip(&clip_params);
            tpt_temporal_stats ts{};
            auto report = [&](int i) {   // (the clip's figures and the display stage, where they are on)
                if (clip) {
                    const tpt_clip_stats cs = hist.clipStats();
                    std::fprintf(stderr, "frame %d: reprojected %llu, clipped %llu, boxed %llu, box %.3f ms\n", i,
                                 (unsigned long long)ts.reprojected, (unsigned long long)cs.clipped,
                                 (unsigned long long)cs.boxed, cs.box_ms);
                }
                if (tonemap) {
                    show(acc.data(), tm);
                    std::fprintf(stderr, "frame %d: exposure scale %.9g (log2 %.9g)\n", i, (double)tms.scale,
                                 (double)tms.log2_scale);
                }
            };
            acc.resize((size_t)W * H * 3);
            var.resize((size_t)W * H);
            len.resize((size_t)W * H);
            std::vector<uint8_t> fb((size_t)W * H * 4, 255);
            const uint64_t base = seed ? seed : (uint64_t)std::time(nullptr);
            for (int i = 0; i < frames; ++i) {
                cam = trucked(yawed(scene.m_camera, yaw * i), truck, i);
                for (const auto& om : motions) {   // (frame 0 keeps the loaded matrices)
                    float m[16];
                    moved_matrix(om, scene.desc().vert_trans + 16 * (size_t)om.object, i, m);
                    if (i > 0) d.setTransforms(om.object, 1, m);
                }
                for (const auto& ow : waves) {
                    std::vector<float> v;
                    waved_vertices(scene.desc(), ow, i, v);
                    d.setVertices(ow.first, (uint32_t)ow.mine.size(), v.data());
                }
                if (!d.built() && refit && i > 0) {
                    tpt_refit_stats rs{};
                    d.refit(&rs);
                    std::fprintf(stderr, "frame %d: refit%s cost %.4f / built %.4f = %.4f, %.3f ms\n", i,
                                 rs.rebuilt ? " (rebuilt)" : "", rs.cost, rs.cost_built,
                                 rs.cost_built > 0.0 ? rs.cost / rs.cost_built : 0.0, rs.ms);
                }
                if (!d.built()) d.build();
                trace(cam, base + (uint64_t)i, false);
                if (temporal_path) {   // the path buffers with their terminal points, every frame
                    std::vector<int32_t> bounces;
                    std::vector<float> points;
                    g = pt.renderAOVPath(d, cam, path_bounces, &bounces, nullptr, &points);
                    ts = pt.temporalPath(hist, cam, f.radiance.data(), g.view(), bounces.data(), points.data(), acc.data(),
                                         var.data(), len.data(), fb.data());
                    report(i);
                    continue;
                }
                g = pt.renderAOV(d, cam);
                if (!waves.empty())
                    ts = pt.temporalDeform(hist, cam, f.radiance.data(), g.view(), acc.data(), var.data(), len.data(),
                                           nullptr, fb.data());
                else if (motions.empty())
                    ts = pt.temporal(hist, cam, f.radiance.data(), g.view(), acc.data(), var.data(), len.data(), fb.data());
                else
                    ts = pt.temporalMotion(hist, cam, f.radiance.data(), g.view(), acc.data(), var.data(), len.data(),
                                           nullptr, fb.data());
                report(i);
            }
            write_pfm(out + "_temporal.pfm", acc, W, H, 3);
            write_ppm(out + "_temporal.ppm", fb, W, H);
        } else if (adaptive) {
            const int tx = (W + 15) / 16, ty = (H + 15) / 16;
            std::vector<int32_t> tile_spp((size_t)tx * ty);
            ad_stats = pt.doTraceAdaptive(d, cam, f.bgra.data(), ad_min, ad_max, ad_target, seed, depth,
                                          f.radiance.data(), tile_spp.data());
            std::vector<float> px((size_t)W * H);
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) px[(size_t)y * W + x] = (float)tile_spp[(size_t)(y / 16) * tx + x / 16];
            write_pfm(out + "_spp.pfm", px, W, H, 1);
        } else {
            for (int i = 0; i < frames; ++i) {
                if (yaw != 0.0 || truck[0] != 0.0 || truck[1] != 0.0 || truck[2] != 0.0)
                    cam = trucked(yawed(scene.m_camera, yaw * i), truck, i);
                trace(cam, seed, progressive && i > 0);
            }
        }
        write_ppm(out + ".ppm", f.bgra, W, H);
        write_pfm(out + ".pfm", f.radiance, W, H, 3);
        if (scale > 1) write_pfm(out + "_low.pfm", low_rad, lo.width, lo.height, 3);
        // --tonemap: the frame the display stage takes, unless a filter below replaces it.  After
        // --temporal the last frame is mapped already; a filtered one is mapped at that frame's scale.
        tpt_tonemap_params tm_last = tm;
        if (tonemap && temporal) {
            tm_last.flags &= ~TPT_TONEMAP_AUTO;
            tm_last.ev = tms.log2_scale;
        }
        std::vector<float> shown;
        if (aov || aov_path || denoise || svgf) {
            if (aov_path) {   // the filters' guides follow the mirrors (the temporal pass above did not)
                std::vector<int32_t> bounces;
                g = pt.renderAOVPath(d, cam, path_bounces, &bounces);
                write_pfm(out + "_bounces.pfm", std::vector<float>(bounces.begin(), bounces.end()), W, H, 1);
            } else if (!temporal) {
                g = pt.renderAOV(d, cam);
            }   // (--temporal-path: g holds the last frame's path guides already)
            if (aov || aov_path) {
                write_pfm(out + "_albedo.pfm", g.albedo, W, H, 3);
                write_pfm(out + "_normal.pfm", g.normal, W, H, 3);
                write_pfm(out + "_depth.pfm", g.depth, W, H, 1);
            }
            if (denoise) {   // of the temporal output when there is one
                std::vector<float> clean((size_t)W * H * 3);
                std::vector<uint8_t> fb((size_t)W * H * 4, 255);
                pt.denoise(d, temporal ? acc.data() : f.radiance.data(), g.view(), clean.data(), fb.data(),
                           tpt::defaultDenoise(dn_iterations));
                write_pfm(out + "_denoised.pfm", clean, W, H, 3);
                write_ppm(out + "_denoised.ppm", fb, W, H);
                if (tonemap) shown = clean;
            }
            if (svgf) {   // of the temporal output, by its variance and history length, when there is one
                std::vector<float> clean((size_t)W * H * 3);
                std::vector<uint8_t> fb((size_t)W * H * 4, 255);
                pt.denoiseSVGF(d, temporal ? acc.data() : f.radiance.data(), g.view(), temporal ? var.data() : nullptr,
                               temporal ? len.data() : nullptr, clean.data(), nullptr, fb.data(),
                               tpt::defaultSVGF(sv_iterations));
                write_pfm(out + "_svgf.pfm", clean, W, H, 3);
                write_ppm(out + "_svgf.ppm", fb, W, H);
                if (tonemap) shown = clean;
            }
        }
        if (tonemap) {
            if (!shown.empty()) show(shown.data(), tm_last);
            else if (!temporal) show(f.radiance.data(), tm);
            if (!temporal)
                std::fprintf(stderr, "exposure scale %.9g (log2 %.9g)\n", (double)tms.scale, (double)tms.log2_scale);
            write_ppm(out + "_display.ppm", display, W, H);
        }
        if (adaptive) {
            std::printf("{\"scene\": \"%s\", \"width\": %d, \"height\": %d, \"target\": %g, \"min_spp\": %d, "
                        "\"max_spp\": %d, \"mean_spp\": %.2f, \"passes\": %d, \"unconverged_tiles\": %d, "
                        "\"rays\": %llu, \"trace_ms\": %.3f, \"error_ms\": %.3f, \"out\": \"%s.ppm\"}\n",
                        scene_file.c_str(), W, H, (double)ad_target, ad_min, ad_max,
                        (double)ad_stats.samples / (double)ad_stats.pixels, ad_stats.passes, ad_stats.unconverged_tiles,
                        (unsigned long long)ad_stats.traversals, ad_stats.trace_ms, ad_stats.error_ms, out.c_str());
            return 0;
        }
        const tpt_stats& s = f.stats;
        std::printf("{\"scene\": \"%s\", \"width\": %d, \"height\": %d, \"spp\": %llu, \"rays\": %llu, "
                    "\"trace_ms\": %.3f, \"mrays_per_s\": %.1f, \"out\": \"%s.ppm\"}\n",
                    scene_file.c_str(), W, H, (unsigned long long)s.accumulated_spp, (unsigned long long)s.traversals,
                    s.trace_ms,
                    s.trace_ms > 0 ? s.traversals / (s.trace_ms * 1e3) : 0.0, out.c_str());
    } catch (const std::exception& e) {
        std::cerr << e.what() << std::endl;   // render() prints and returns (path_tracer.cu:575-578)
        return 1;
    }
    return 0;
}
