// rz_editor.hip -- RayZen's editor preview (main.cpp:1210-1322, shaders/editor_{vertex,fragment}.glsl) as a ray cast
// (include/rayzen_hip.h: rz_render_editor).
//
// The reference rasterises every mesh with a depth test and shades each fragment with editor_fragment.glsl: GGX direct
// lighting and an ambient term, no shadows.  For a pinhole camera the visible surface of a pixel is the closest hit of the
// ray through its centre, so the mode needs no raster pipeline: one lane per pixel,
//   1. the render's camera ray with a jitter of zero (rz_path.h: camera_ray_centre), from cam_pos;
//   2. the render's own closest-hit query (rz_query.h: ray_query -> trace_closest, or trace_spread under
//      RZ_EDITOR_INCOHERENT), with the winning triangle (TraceExtra) as rz_trace_rays_kernel returns it;
//   3. the rasteriser's clipping: the hit through view, then proj (float32, in GLM's order) must satisfy -w <= z <= w.
//      Beyond the far plane the pixel is background (whatever lies farther is clipped as well); in front of the near plane
//      the surface is skipped by restarting the query where the ray crosses the near plane, at most RZ_EDITOR_RESTARTS times;
//   4. editor_fragment.glsl statement by statement (editor_shade, in binary64), with N = normalize(the hit's world normal);
//   5. the clear colour where nothing visible was hit.
// A wave covers 64 pixels of one row per step of a grid-stride loop over a persistent grid of one-wave workgroups, as
// rz_rays.hip (or one 8 x 8 tile, RZ_TILE_W x RZ_TILE_H, under RZ_EDITOR_TILES=1: the rows measured faster on C2, C4 and C5,
// the tiles on c2close and RayZen's own scene -- profiles/editor/README.md).  Nothing of the render state is touched (accumulation, currentIor, pools, the claim counter,
// the frame of rz_set_frame); a walk stopped at its backstop sets RZ_BACKSTOP_RAYS, as the ray queries do.
// Shared with the other off-frame passes: the pixel's ray (rz_pixel_cast.h: pixel_centre_dir) and the rz_hit record (rz_query.h:
// store_hit).
#include "rz_internal.h"
#include "rz_pixel_cast.h"

namespace rz {

#ifndef RZ_EDITOR_RESTARTS
#define RZ_EDITOR_RESTARTS 4        // near-plane restarts of one pixel; one suffices unless rounding puts the crossing short
#endif

// GLM 0.9.9's mat4 * vec4, rows 2 and 3 only: (m0 x + m1 y) + (m2 z + m3 w), m column-major
__device__ __forceinline__ float glm_row(const float* m, int r, float x, float y, float z, float w) {
    return (m[r] * x + m[4 + r] * y) + (m[8 + r] * z + m[12 + r] * w);
}
// proj * (view * (v, w)): the clip-space z and w of a point (w = 1) or a direction (w = 0)
__device__ __forceinline__ float2 clip_zw(const EditorLaunch& E, v3 v, float w) {
    const float* V = E.view;
    const float ex = glm_row(V, 0, v.x, v.y, v.z, w), ey = glm_row(V, 1, v.x, v.y, v.z, w);
    const float ez = glm_row(V, 2, v.x, v.y, v.z, w), ew = glm_row(V, 3, v.x, v.y, v.z, w);
    return make_float2(glm_row(E.proj, 2, ex, ey, ez, ew), glm_row(E.proj, 3, ex, ey, ez, ew));
}

// editor_fragment.glsl:58-112 for the surface point p with the world normal n and material index mat, evaluated in binary64
// and rounded to binary32 once at the end.  In binary32 the GGX lobe of a low roughness is ill-conditioned where the
// reference's clamp puts the mirror and glass materials (roughness 0.05: a2 = 6.25e-6): near the highlight denom =
// NdotH^2 (a2 - 1) + 1 is of the order of a2, so the rounding of V, L, H and NdotH alone moves D by up to several percent.
// Binary64 keeps the colour within a few binary32 ulps of the exact value of the shader's formula for the given hit, at a
// cost that is small beside the traversal: it runs once per visible pixel and light, after the query.
struct d3 { double x, y, z; };
__device__ __forceinline__ d3 mkd(double x, double y, double z) { d3 r; r.x = x; r.y = y; r.z = z; return r; }
__device__ __forceinline__ d3 mkd(v3 v) { return mkd(v.x, v.y, v.z); }
__device__ __forceinline__ d3 operator+(d3 a, d3 b) { return mkd(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ d3 operator-(d3 a, d3 b) { return mkd(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ d3 operator*(d3 a, d3 b) { return mkd(a.x * b.x, a.y * b.y, a.z * b.z); }
__device__ __forceinline__ d3 operator*(d3 a, double s) { return mkd(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ d3 operator/(d3 a, double s) { return mkd(a.x / s, a.y / s, a.z / s); }
__device__ __forceinline__ double dotd(d3 a, d3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ double lengthd(d3 a) { return __builtin_sqrt(dotd(a, a)); }
__device__ __forceinline__ d3 normalized(d3 a) { return a / lengthd(a); }
__device__ __forceinline__ double mixd(double a, double b, double t) { return a * (1.0 - t) + b * t; }

// editor_fragment.glsl:46-56 (the constants as written: 3.14159, 1e-4, 1e-6, in binary32 as the shader's literals are)
__device__ __forceinline__ double distribution_ggx(double NdotH, double roughness) {
    const double a = roughness * roughness;
    const double a2 = a * a;
    const double denom = (NdotH * NdotH) * (a2 - 1.0) + 1.0;
    return a2 / __builtin_fmax((double)3.14159f * denom * denom, (double)1e-4f);
}
__device__ __forceinline__ double geometry_schlick_ggx(double NdotV, double roughness) {
    const double r = roughness + 1.0;
    const double k = (r * r) / 8.0;
    return NdotV / (NdotV * (1.0 - k) + k + (double)1e-6f);
}

// (What stays live across the light loop is kept small -- the material and the sum in binary32, only N and V in binary64 --
//  so that the kernel fits its 128 VGPRs without a spill: the sum of a handful of terms loses nothing the tolerance sees.)
__device__ __forceinline__ v3 editor_shade(const KParams& K, const EditorLaunch& E, v3 pf, v3 n, int mat) {
    // clamp(materialIndex, 0, materials.length() - 1); (an upload with an index out of range is refused -- RZ_ERR_BAD_SCENE --
    // so the clamp is the shader's statement more than a case that occurs)
    const int matIndex = min(max(mat, 0), K.nMaterials - 1);
    const DevMaterial m = K.materials[matIndex];
    const v3 albedo = mk3(m.albedo[0], m.albedo[1], m.albedo[2]);
    const d3 N = normalized(mkd(n));
    const d3 V = normalized(mkd(K.camPos[0], K.camPos[1], K.camPos[2]) - mkd(pf));
    const double NdotV = __builtin_fmax(dotd(N, V), 0.0);            // no flip toward the viewer: a back face gets 0
    v3 color = mk3(E.ambient[0] * albedo.x, E.ambient[1] * albedo.y, E.ambient[2] * albedo.z);
    for (int i = 0; i < K.nLights; ++i) {          // min(numLights, lights.length())
        const DevLight light = K.lights[i];
        d3 L;
        double attenuation;
        if (light.posdir[3] == 1.0f) {
            const d3 lightVec = mkd(light.posdir[0], light.posdir[1], light.posdir[2]) - mkd(pf);
            const double distance = __builtin_fmax(lengthd(lightVec), (double)0.001f);
            L = lightVec / distance;
            attenuation = (double)light.power / (distance * distance);
        } else {
            L = normalized(mkd(light.posdir[0], light.posdir[1], light.posdir[2]));
            attenuation = light.power;
        }
        const double NdotL = __builtin_fmax(dotd(N, L), 0.0);
        if (NdotL <= 0.0) continue;
        const d3 H = normalized(V + L);
        const double NdotH = __builtin_fmax(dotd(N, H), 0.0);
        const double VdotH = __builtin_fmax(dotd(V, H), 0.0);
        const double rough = __builtin_fmin(__builtin_fmax((double)m.roughness, (double)0.05f), 1.0);
        const double D = distribution_ggx(NdotH, rough);
        const double G = geometry_schlick_ggx(NdotV, rough) * geometry_schlick_ggx(NdotL, rough);
        const double metallic = m.metallic;
        const d3 alb = mkd(albedo);
        const d3 F0 = mkd(mixd((double)0.04f, alb.x, metallic), mixd((double)0.04f, alb.y, metallic), mixd((double)0.04f, alb.z, metallic));
        const double q = 1.0 - VdotH, q2 = q * q, q5 = q2 * q2 * q;                  // fresnelSchlick (FS:533-535)
        const d3 F = F0 + (mkd(1.0, 1.0, 1.0) - F0) * q5;
        const d3 numerator = F * (D * G);
        const double denominator = __builtin_fmax(4.0 * NdotV * NdotL, (double)1e-4f);
        const d3 specular = numerator / denominator;
        const d3 kD = (mkd(1.0, 1.0, 1.0) - F) * (1.0 - metallic);
        const d3 diffuse = (kD * alb) / (double)3.14159f;
        const d3 add = (diffuse + specular) * mkd(light.color[0], light.color[1], light.color[2]) * attenuation * NdotL;
        color = color + mk3((float)add.x, (float)add.y, (float)add.z);
    }
    if (m.transparency > 0.0f) {        // mix(color, albedo, clamp(transparency, 0, 1) * 0.5)
        const float t = clamp_(m.transparency, 0.0f, 1.0f) * 0.5f;
        color = mk3(mix_(color.x, albedo.x, t), mix_(color.y, albedo.y, t), mix_(color.z, albedo.z, t));
    }
    return color;
}

template <bool OVF, bool SPREAD>
__global__ __launch_bounds__(64, RZ_RAYS_MIN_WAVES) void rz_editor_kernel(const KParams K, const EditorLaunch E) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const BlasStackT<OVF> bstk = rays_stack<OVF>(K, lds_raw);
    const int lane = threadIdx.x & 63;
    const v3 cam = mk3(K.camPos[0], K.camPos[1], K.camPos[2]);
    bool cut = false;
    for (long long u = blockIdx.x; u < E.units; u += gridDim.x) {
        const int uy = (int)(u / E.unitsX), ux = (int)(u - (long long)uy * E.unitsX);
        const int px = E.rows ? ux * 64 + lane : ux * RZ_TILE_W + (lane & 7);
        const int py = E.rows ? uy : uy * RZ_TILE_H + (lane >> 3);
        const bool inside = px < K.width && py < K.height;
        v3 d = mk3(0.0f, 0.0f, 0.0f);
        if (inside) d = pixel_centre_dir(K, px, py, K.width, K.height);
        // the closest hit, and past the near plane when it lies in front of it
        HitRec h;
        int tri = -1, restarts = 0;
        float start = 0.0f;                 // distance along the camera ray the query started from (0: the camera itself)
        bool run = inside, visible = false;
        while (rz_ballot(run) != 0ull) {
            if (run) {
                const v3 o = start > 0.0f ? cam + d * start : cam;
                TraceExtra x;
                const bool found = ray_query<OVF, SPREAD>(K, o, d, h, bstk, x);
                cut = cut || x.cut;
                run = false;
                if (found) {
                    const float2 c = clip_zw(E, h.p, 1.0f);
                    if (-c.y <= c.x && c.x <= c.y) {
                        visible = true;
                        tri = x.tri;
                    } else if (c.x < -c.y && restarts < RZ_EDITOR_RESTARTS) {
                        // in front of the near plane: z + w is linear along the ray, zero where it crosses the plane
                        const float2 c0 = clip_zw(E, cam, 1.0f), c1 = clip_zw(E, d, 0.0f);
                        const float tNear = -(c0.x + c0.y) / (c1.x + c1.y);
                        start = fmax_(start + h.t, tNear);
                        restarts += 1;
                        run = true;
                    }               // beyond the far plane (or a NaN): background, and what lies farther is clipped too
                }
            }
        }
        if (!inside) continue;
        const size_t pix = (size_t)py * K.width + px;
        // rz_trace_rays' record, t from the camera (written before the shading, which then has the record's registers to itself)
        if (E.hits) store_hit(K, E.instTriOff, E.hits, pix, visible, h, tri, start > 0.0f ? start + h.t : h.t);
        if (!E.rgb32f && !E.rgba8) continue;
        const v3 color = visible ? editor_shade(K, E, h.p, h.n, h.mat) : mk3(E.clear[0], E.clear[1], E.clear[2]);
        if (E.rgb32f) {
            E.rgb32f[3 * pix] = color.x;
            E.rgb32f[3 * pix + 1] = color.y;
            E.rgb32f[3 * pix + 2] = color.z;
        }
        if (E.rgba8)        // rz_present_kernel's quantisation
            E.rgba8[pix] = make_uchar4((unsigned char)__builtin_rintf(clamp_(color.x, 0.0f, 1.0f) * 255.0f),
                                       (unsigned char)__builtin_rintf(clamp_(color.y, 0.0f, 1.0f) * 255.0f),
                                       (unsigned char)__builtin_rintf(clamp_(color.z, 0.0f, 1.0f) * 255.0f), 255);
    }
    rays_backstop(E.errWord, cut);
}

void launch_editor(const KParams& K, const EditorLaunch& E, hipStream_t stream) {
    const dim3 g((unsigned)E.grid), b(64);
    const size_t lds = (size_t)K.blasStackCap * 64 * sizeof(uint2);
    const bool ovf = K.blasOvfCap > 0;
    if (ovf) {
        if (E.spread) hipLaunchKernelGGL((rz_editor_kernel<true, true>), g, b, lds, stream, K, E);
        else hipLaunchKernelGGL((rz_editor_kernel<true, false>), g, b, lds, stream, K, E);
    } else {
        if (E.spread) hipLaunchKernelGGL((rz_editor_kernel<false, true>), g, b, lds, stream, K, E);
        else hipLaunchKernelGGL((rz_editor_kernel<false, false>), g, b, lds, stream, K, E);
    }
}

}  // namespace rz
