// motion.cpp -- tpt_motion_matrices: what k_temporal with MotionArgs (post.hip) needs to follow an
// object from this frame's world into the previous frame's (DESIGN.md section 5 "Moving
// objects").  Host only, no HIP: double arithmetic, each entry rounded to float once.
#include <cmath>
#include <cstring>

#include "tpt.h"

namespace {

constexpr int kRecordFloats = 24;   // device_api.hpp kMotionRecordFloats
constexpr int32_t kTracked = 0, kIdentity = 1, kUntracked = 2;

// Inverse of a 3x3 matrix (row-major) by cofactors; false: the determinant is 0 or not finite.
bool invert3(const double* a, double* inv) {
    const double c00 = a[4] * a[8] - a[5] * a[7], c01 = a[5] * a[6] - a[3] * a[8], c02 = a[3] * a[7] - a[4] * a[6];
    const double det = a[0] * c00 + a[1] * c01 + a[2] * c02;
    if (!(std::fabs(det) > 0.0) || !std::isfinite(det)) return false;
    inv[0] = c00 / det;
    inv[1] = (a[2] * a[7] - a[1] * a[8]) / det;
    inv[2] = (a[1] * a[5] - a[2] * a[4]) / det;
    inv[3] = c01 / det;
    inv[4] = (a[0] * a[8] - a[2] * a[6]) / det;
    inv[5] = (a[2] * a[3] - a[0] * a[5]) / det;
    inv[6] = c02 / det;
    inv[7] = (a[1] * a[6] - a[0] * a[7]) / det;
    inv[8] = (a[0] * a[4] - a[1] * a[3]) / det;
    return true;
}

bool affine(const float* m) { return m[3] == 0.0f && m[7] == 0.0f && m[11] == 0.0f && m[15] == 1.0f; }

void write_identity(float* out) {
    static const float unit[21] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1};
    std::memcpy(out, unit, sizeof unit);
}

// D (rows of 4) and G (rows of 3) of one object; false: untracked
bool track(const float* prev, const float* cur, float* out) {
    if (!affine(prev) || !affine(cur)) return false;
    double a[9], ap[9], t[3], tp[3];   // the linear parts row-major, the translations
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) {
            a[3 * r + c] = (double)cur[4 * c + r];
            ap[3 * r + c] = (double)prev[4 * c + r];
        }
        t[r] = (double)cur[12 + r];
        tp[r] = (double)prev[12 + r];
    }
    double ai[9], d[9], dt[3], di[9];
    if (!invert3(a, ai)) return false;   // M is singular
    // M' M^-1 = [A' A^-1 | t' - A' A^-1 t]
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) d[3 * r + c] = ap[3 * r] * ai[c] + ap[3 * r + 1] * ai[3 + c] + ap[3 * r + 2] * ai[6 + c];
    for (int r = 0; r < 3; ++r) dt[r] = tp[r] - (d[3 * r] * t[0] + d[3 * r + 1] * t[1] + d[3 * r + 2] * t[2]);
    if (!invert3(d, di)) return false;   // M' is singular: no normal transform
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) {
            out[4 * r + c] = (float)d[3 * r + c];
            out[12 + 3 * r + c] = (float)di[3 * c + r];   // the inverse, transposed
        }
        out[4 * r + 3] = (float)dt[r];
    }
    for (int i = 0; i < 21; ++i)
        if (!std::isfinite(out[i])) return false;
    return true;
}

}  // namespace

extern "C" int32_t tpt_motion_matrices(uint32_t n_objects, const float* prev16, const float* cur16, float* out24) {
    if (n_objects > 0 && (!prev16 || !cur16 || !out24)) return -1;
    int32_t untracked = 0;
    for (uint32_t o = 0; o < n_objects; ++o) {
        const float* prev = prev16 + 16 * (size_t)o;
        const float* cur = cur16 + 16 * (size_t)o;
        float* out = out24 + kRecordFloats * (size_t)o;
        int32_t flag = kTracked;
        if (std::memcmp(prev, cur, 16 * sizeof(float)) == 0) {
            flag = kIdentity;
            write_identity(out);
        } else if (!track(prev, cur, out)) {
            flag = kUntracked;
            write_identity(out);   // never read by the kernel; a defined value all the same
            ++untracked;
        }
        std::memcpy(out + 21, &flag, sizeof flag);
        out[22] = 0.0f;
        out[23] = 0.0f;
    }
    return untracked;
}
