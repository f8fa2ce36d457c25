// rz_outline.hip -- marks a set of instances on an image (include/rayzen_hip.h: rz_outline).  It reads an id image and a bit set
// and blends a colour into the pixels just outside the selected region, in place; it reads no scene and no frame.
//
//   rz_outline_kernel   a workgroup of 32 x 8 lanes per 32 x 8 pixels, the tiles numbered row by row in a one-dimensional grid.
//                       It stages sel(q) of its tile and a halo of RZ_OUTLINE_MAX_RADIUS pixels in LDS, one byte per pixel (the
//                       test's answer, not the id, so that the word load happens once per id): sel(q) = 0 <= ids[q] < n_instances and bit
//                       ids[q] & 31 of selected[ids[q] >> 5], one word load per id and none for an id out of range; a pixel
//                       outside the image is staged as unselected, which is the rule's "q inside the image".  A workgroup whose
//                       staged pixels are all unselected ends there (most of a frame).  Otherwise a lane whose own pixel is
//                       unselected looks for a selected pixel within `radius` in LDS and, if there is one, blends:
//                       o = in * (1 - alpha) + color * alpha per channel, binary32, one rounding per operation (the library is
//                       compiled without contraction); rgba8: in = (float)byte / 255.0f, out = rint(clamp(o, 0, 1) * 255) as
//                       rz_present_kernel quantises, the alpha byte kept.  Every other pixel is not written.
#include "rz_internal.h"
#include "rz_device_math.h"

namespace rz {

constexpr int OL_W = 32, OL_H = 8, OL_R = RZ_OUTLINE_MAX_RADIUS;
constexpr int OL_SW = OL_W + 2 * OL_R, OL_SH = OL_H + 2 * OL_R;

__global__ __launch_bounds__(OL_W * OL_H) void rz_outline_kernel(const OutlineLaunch O) {
    __shared__ unsigned char sel[OL_SH][OL_SW];
    const int tileY = (int)(blockIdx.x / (unsigned)O.tilesX), tileX = (int)(blockIdx.x - (unsigned)tileY * (unsigned)O.tilesX);
    const int bx = tileX * OL_W, by = tileY * OL_H;
    const int tid = threadIdx.y * OL_W + threadIdx.x;
    int any = 0;
    for (int e = tid; e < OL_SW * OL_SH; e += OL_W * OL_H) {
        const int sy = e / OL_SW, sx = e - sy * OL_SW;
        const int qx = bx + sx - OL_R, qy = by + sy - OL_R;
        unsigned char s = 0;
        if (qx >= 0 && qx < O.width && qy >= 0 && qy < O.height) {
            const int id = O.ids[(size_t)qy * O.width + qx];
            if (id >= 0 && (unsigned long long)id < O.nInstances) s = (unsigned char)((O.selected[id >> 5] >> (id & 31)) & 1u);
        }
        sel[sy][sx] = s;
        any |= s;
    }
    if (!__syncthreads_or(any)) return;
    const int px = bx + threadIdx.x, py = by + threadIdx.y;
    if (px >= O.width || py >= O.height) return;
    const int cx = threadIdx.x + OL_R, cy = threadIdx.y + OL_R;
    if (sel[cy][cx]) return;
    int found = 0;
    for (int dy = -O.radius; dy <= O.radius; ++dy)
        for (int dx = -O.radius; dx <= O.radius; ++dx) found |= sel[cy + dy][cx + dx];
    if (!found) return;
    const size_t p = (size_t)py * O.width + px;
    const float keep = 1.0f - O.alpha;
    if (O.rgb) {
        O.rgb[3 * p] = O.rgb[3 * p] * keep + O.color[0] * O.alpha;
        O.rgb[3 * p + 1] = O.rgb[3 * p + 1] * keep + O.color[1] * O.alpha;
        O.rgb[3 * p + 2] = O.rgb[3 * p + 2] * keep + O.color[2] * O.alpha;
    }
    if (O.rgba8) {
        const uchar4 b = O.rgba8[p];
        const float r = ((float)b.x / 255.0f) * keep + O.color[0] * O.alpha;
        const float g = ((float)b.y / 255.0f) * keep + O.color[1] * O.alpha;
        const float bl = ((float)b.z / 255.0f) * keep + O.color[2] * O.alpha;
        O.rgba8[p] = make_uchar4((unsigned char)__builtin_rintf(clamp_(r, 0.0f, 1.0f) * 255.0f),
                                 (unsigned char)__builtin_rintf(clamp_(g, 0.0f, 1.0f) * 255.0f),
                                 (unsigned char)__builtin_rintf(clamp_(bl, 0.0f, 1.0f) * 255.0f), b.w);
    }
}

void launch_outline(OutlineLaunch O, hipStream_t stream) {
    O.tilesX = (O.width + OL_W - 1) / OL_W;
    const dim3 g((unsigned)O.tilesX * (unsigned)((O.height + OL_H - 1) / OL_H)), b(OL_W, OL_H);     // (one dimension: no 65535-row limit)
    hipLaunchKernelGGL(rz_outline_kernel, g, b, 0, stream, O);
}

}  // namespace rz
