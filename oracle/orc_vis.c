/* orc_vis.c -- CPU oracle (TEST INFRASTRUCTURE ONLY, see orc.h) of the colour image of the visual meshes.
 *
 * Stands where the reference draws its cameras through MuJoCo's OpenGL renderer (gym_guided_vision/gym_guided_vision/env.py:180-188
 * get_obs "pixels", :195-200 render [EXT]); like the device's rasteriser (av_aloha_amd/csrc/avsim_vis.hip.h) it draws the decimated
 * visual scene of compiler/vismesh.py with flat Lambert shading, and PARITY with the reference's OpenGL pixels is UNPINNED.
 * What it checks is the device's projection / clipping / binning / depth test: here every pixel's ray is intersected with every
 * triangle that faces the camera (Moeller-Trumbore, f64, depth along the optical axis >= znear), no projection and no tiles.
 *
 * The caller passes the expanded scene (tests: vismesh.expand_instances) and the body poses of an orc_data. */
#include <math.h>
#include <stdlib.h>

#include "orc.h"

static void vquat2mat(const double* q, double* R) {
    double w = q[0], x = q[1], y = q[2], z = q[3];
    R[0] = w * w + x * x - y * y - z * z; R[1] = 2 * (x * y - w * z); R[2] = 2 * (x * z + w * y);
    R[3] = 2 * (x * y + w * z); R[4] = w * w - x * x + y * y - z * z; R[5] = 2 * (y * z - w * x);
    R[6] = 2 * (x * z - w * y); R[7] = 2 * (y * z + w * x); R[8] = w * w - x * x - y * y + z * z;
}

static unsigned char vq8(double x) { x = x < 0 ? 0 : (x > 1 ? 1 : x); return (unsigned char)(x * 255.0 + 0.5); }

/* Light-space frame of the directional light: e1, e2 span the plane normal to the (unit) light direction lw.  The device builds its shadow
 * map in the same frame (avsim_vis.hip.h vis_light_frame). */
static void light_frame(const double* lw, double* e1, double* e2) {
    const double ax[3] = {fabs(lw[0]) < 0.9 ? 1.0 : 0.0, fabs(lw[0]) < 0.9 ? 0.0 : 1.0, 0.0};
    double d = ax[0] * lw[0] + ax[1] * lw[1] + ax[2] * lw[2];
    for (int k = 0; k < 3; k++) e1[k] = ax[k] - d * lw[k];
    d = sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]);
    for (int k = 0; k < 3; k++) e1[k] /= d;
    e2[0] = lw[1] * e1[2] - lw[2] * e1[1]; e2[1] = lw[2] * e1[0] - lw[0] * e1[2]; e2[2] = lw[0] * e1[1] - lw[1] * e1[0];
}

/* What shading a fragment needs of a render call: the camera-frame vertices vc, the camera's rotation Rc, the light's direction lc and the
 * world's up in the camera frame, the scene's tables. */
typedef struct {
    const orc_data* d;
    const double *vc, *Rc, *L, *rgb, *uv, *tnorm;
    const int *tri, *vbody, *tex, *texel;
    int texn;
    double lc[3], up[3];
} vis_shader;

/* cosine between the outward normal of triangle t and the direction to the light (flat; > 0: the face is turned towards the light) */
static double vis_light_cos(const vis_shader* s, int t) {
    const double *a = s->vc + 3 * s->tri[3 * t], *bb = s->vc + 3 * s->tri[3 * t + 1], *c = s->vc + 3 * s->tri[3 * t + 2];
    const double n[3] = {(bb[1] - a[1]) * (c[2] - a[2]) - (bb[2] - a[2]) * (c[1] - a[1]), (bb[2] - a[2]) * (c[0] - a[0]) - (bb[0] - a[0]) * (c[2] - a[2]),
                         (bb[0] - a[0]) * (c[1] - a[1]) - (bb[1] - a[1]) * (c[0] - a[0])};
    return -(n[0] * s->lc[0] + n[1] * s->lc[1] + n[2] * s->lc[2]) / sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
}

/* col[3], not yet quantised: the fragment of triangle bt (< 0: the sky) where the ray dir hits it at barycentrics (bu, bv); shadowed: the
 * directional light's diffuse and specular terms go */
static void vis_shade(const vis_shader* s, int bt, double bu, double bv, const double* dir, int shadowed, double* col) {
    const orc_data* d = s->d;
    const double *vc = s->vc, *Rc = s->Rc, *L = s->L, *rgb = s->rgb, *uv = s->uv, *tnorm = s->tnorm, *lc = s->lc, *up = s->up;
    const int *tri = s->tri, *vbody = s->vbody, *tex = s->tex, *texel = s->texel, texn = s->texn;
    const double amb = L[0], hd = L[1], ld = L[2];
    if (bt >= 0) {
        const double *a = vc + 3 * tri[3 * bt], *bb = vc + 3 * tri[3 * bt + 1], *c = vc + 3 * tri[3 * bt + 2];
        double n[3] = {(bb[1] - a[1]) * (c[2] - a[2]) - (bb[2] - a[2]) * (c[1] - a[1]), (bb[2] - a[2]) * (c[0] - a[0]) - (bb[0] - a[0]) * (c[2] - a[2]),
                       (bb[0] - a[0]) * (c[1] - a[1]) - (bb[1] - a[1]) * (c[0] - a[0])};
        const double g[3] = {(a[0] + bb[0] + c[0]) / 3, (a[1] + bb[1] + c[1]) / 3, (a[2] + bb[2] + c[2]) / 3};
        const double nn = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]), gg = sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
        const double ch = -(n[0] * g[0] + n[1] * g[1] + n[2] * g[2]) / (nn * gg);     /* headlight term at the centroid: flat per triangle */
        double cl = -(n[0] * lc[0] + n[1] * lc[1] + n[2] * lc[2]) / nn;
        if (shadowed) cl = 0;
        const int in_shadow = cl == 0;      /* (set by the shadow ray above; a face turned away from the light has cl < 0) */
        double lum = amb + hd * ch + ld * (cl > 0 ? cl : 0);
        if (lum > 1) lum = 1;
        /* the light's specular term (render_light[16] = light specular x material specular, [17] the exponent): Blinn's half vector with
         * the viewer at infinity along the optical axis, as fixed-function GL has it [EXT]; white, added to every channel; gone in shadow */
        double spec = 0;
        if (cl > 0 && L[16] > 0) {
            double h[3] = {-lc[0], -lc[1], -lc[2] + 1.0};
            const double hn = sqrt(h[0] * h[0] + h[1] * h[1] + h[2] * h[2]);
            if (hn > 1e-12) {
                double sgn = ch >= 0 ? 1.0 : -1.0;          /* the normal turned towards the camera */
                const double nh = sgn * (n[0] * h[0] + n[1] * h[1] + n[2] * h[2]) / (nn * hn);
                if (nh > 0) spec = L[16] * pow(nh, L[17]);
            }
        }
        if (tnorm) {
            /* smooth shading: the corners' own shades, interpolated at the hit point (1 - u - v, u, v) */
            const double* Rbd = d->xmat + 9 * vbody[tri[3 * bt]];
            const double* P3[3] = {a, bb, c};
            double at[3][3];
            for (int k = 0; k < 3; k++) {
                const double* tn = tnorm + 9 * (size_t)bt + 3 * k;
                double nw[3], nc[3];
                for (int i = 0; i < 3; i++) nw[i] = Rbd[3 * i] * tn[0] + Rbd[3 * i + 1] * tn[1] + Rbd[3 * i + 2] * tn[2];
                for (int j = 0; j < 3; j++) nc[j] = Rc[j] * nw[0] + Rc[3 + j] * nw[1] + Rc[6 + j] * nw[2];
                const double* p = P3[k];
                const double pl = sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
                double chv = -(nc[0] * p[0] + nc[1] * p[1] + nc[2] * p[2]) / (pl > 1e-300 ? pl : 1e-300);
                if (chv < 0) chv = 0;
                const double clv = -(nc[0] * lc[0] + nc[1] * lc[1] + nc[2] * lc[2]);
                at[k][0] = amb + hd * chv + ld * (clv > 0 ? clv : 0); if (at[k][0] > 1) at[k][0] = 1;
                at[k][1] = amb + hd * chv; if (at[k][1] > 1) at[k][1] = 1;
                at[k][2] = 0;
                if (clv > 0 && L[16] > 0) {
                    double h[3] = {-lc[0], -lc[1], -lc[2] + 1.0};
                    const double hn = sqrt(h[0] * h[0] + h[1] * h[1] + h[2] * h[2]);
                    const double nh = hn > 1e-12 ? (nc[0] * h[0] + nc[1] * h[1] + nc[2] * h[2]) / hn : 0;
                    if (nh > 0) at[k][2] = L[16] * pow(nh, L[17]);
                }
            }
            const double b0 = 1.0 - bu - bv;
            lum = b0 * at[0][in_shadow ? 1 : 0] + bu * at[1][in_shadow ? 1 : 0] + bv * at[2][in_shadow ? 1 : 0];
            spec = in_shadow ? 0.0 : b0 * at[0][2] + bu * at[1][2] + bv * at[2][2];
            if (lum < 0) lum = 0;
            if (lum > 1) lum = 1;
            if (spec < 0) spec = 0;
        }
        if (tex[bt]) {
            const double* w = uv + 6 * bt;
            const double tu = w[0] + bu * (w[2] - w[0]) + bv * (w[4] - w[0]), tv = w[1] + bu * (w[3] - w[1]) + bv * (w[5] - w[1]);
            const double fu = tu - floor(tu), fv = tv - floor(tv);
            int xi = (int)(fu * texn), yi = (int)((1.0 - fv) * texn);
            xi = xi > texn - 1 ? texn - 1 : xi; yi = yi > texn - 1 ? texn - 1 : yi;
            const unsigned px = (unsigned)texel[yi * texn + xi];
            col[0] = (px & 255u) / 255.0 * lum + spec; col[1] = ((px >> 8) & 255u) / 255.0 * lum + spec; col[2] = ((px >> 16) & 255u) / 255.0 * lum + spec;
        } else
            for (int k = 0; k < 3; k++) col[k] = rgb[3 * bt + k] * lum + spec;
    } else {
        const double idn = 1.0 / sqrt(dir[0] * dir[0] + dir[1] * dir[1] + 1.0);
        const double w = 0.5 + 0.5 * (up[0] * dir[0] + up[1] * dir[1] - up[2]) * idn;
        for (int k = 0; k < 3; k++) col[k] = L[12 + k] + (L[8 + k] - L[12 + k]) * w;
    }
}

/* One camera's view of the scene in the current state: camera pose, the light's frame and shadow box, the vertices in the camera frame
 * (vc) and the world frame (vw), which triangles face the camera. */
typedef struct {
    double Rc[9], pc[3], lw[3], lc[3], up[3], e1[3], e2[3], znear, scale, sh_s, sh_t;
    double *vc, *vw;
    unsigned char* front;
} vis_view;

static void vis_view_free(vis_view* V) { free(V->vc); free(V->front); }

static int vis_view_init(vis_view* V, const orc_data* d, int cam, int H, int nvert, const double* vert, const int* vbody, int ntri, const int* tri) {
    const orc_model* m = d->m;
    int b = m->cam_body[cam];
    double Rl[9], *Rc = V->Rc, *pc = V->pc, *lw = V->lw;
    vquat2mat(m->cam_quat + 4 * cam, Rl);
    const double *Rb = d->xmat + 9 * b, *pb = d->xpos + 3 * b, *cp = m->cam_pos + 3 * cam;
    for (int i = 0; i < 3; i++) {
        pc[i] = pb[i] + Rb[3 * i] * cp[0] + Rb[3 * i + 1] * cp[1] + Rb[3 * i + 2] * cp[2];
        for (int j = 0; j < 3; j++) Rc[3 * i + j] = Rb[3 * i] * Rl[j] + Rb[3 * i + 1] * Rl[3 + j] + Rb[3 * i + 2] * Rl[6 + j];
    }
    V->znear = m->cam_clip[0];
    V->scale = 2.0 * tan(0.5 * m->cam_fovy[cam] * 3.14159265358979323846 / 180.0) / H;
    const double* L = m->render_light;
    const double ln = sqrt(L[4] * L[4] + L[5] * L[5] + L[6] * L[6]);
    for (int j = 0; j < 3; j++) lw[j] = L[4 + j] / ln;
    for (int j = 0; j < 3; j++) {
        V->lc[j] = Rc[j] * lw[0] + Rc[3 + j] * lw[1] + Rc[6 + j] * lw[2];     /* light direction, world up: camera frame */
        V->up[j] = Rc[6 + j];
    }
    light_frame(lw, V->e1, V->e2);
    const double sh_c[3] = {L[7], L[11], L[15]};
    V->sh_s = sh_c[0] * V->e1[0] + sh_c[1] * V->e1[1] + sh_c[2] * V->e1[2];
    V->sh_t = sh_c[0] * V->e2[0] + sh_c[1] * V->e2[1] + sh_c[2] * V->e2[2];
    /* vertices into the camera frame (and the world frame, for the shadow rays) */
    double* vc = V->vc = (double*)malloc(sizeof(double) * 6 * (size_t)nvert);
    V->front = (unsigned char*)malloc((size_t)ntri + 1);
    if (!vc || !V->front) { vis_view_free(V); return -2; }
    double* vw = V->vw = vc + 3 * (size_t)nvert;
    for (int v = 0; v < nvert; v++) {
        const double *R = d->xmat + 9 * vbody[v], *p = d->xpos + 3 * vbody[v], *x = vert + 3 * v;
        double w[3];
        for (int i = 0; i < 3; i++) { vw[3 * v + i] = R[3 * i] * x[0] + R[3 * i + 1] * x[1] + R[3 * i + 2] * x[2] + p[i]; w[i] = vw[3 * v + i] - pc[i]; }
        for (int j = 0; j < 3; j++) vc[3 * v + j] = Rc[j] * w[0] + Rc[3 + j] * w[1] + Rc[6 + j] * w[2];
    }
    /* a triangle faces the camera when its outward normal points against the direction from the eye to its centroid */
    for (int t = 0; t < ntri; t++) {
        const double *a = vc + 3 * tri[3 * t], *bb = vc + 3 * tri[3 * t + 1], *c = vc + 3 * tri[3 * t + 2];
        const double n[3] = {(bb[1] - a[1]) * (c[2] - a[2]) - (bb[2] - a[2]) * (c[1] - a[1]), (bb[2] - a[2]) * (c[0] - a[0]) - (bb[0] - a[0]) * (c[2] - a[2]),
                             (bb[0] - a[0]) * (c[1] - a[1]) - (bb[1] - a[1]) * (c[0] - a[0])};
        V->front[t] = n[0] * (a[0] + bb[0] + c[0]) + n[1] * (a[1] + bb[1] + c[1]) + n[2] * (a[2] + bb[2] + c[2]) < 0;
    }
    return 0;
}

static vis_shader vis_shader_of(const vis_view* V, const orc_data* d, const int* tri, const int* vbody, const double* rgb, const double* uv, const int* tex,
                                const int* texel, int texn, const double* tnorm) {
    vis_shader s = {d, V->vc, V->Rc, d->m->render_light, rgb, uv, tnorm, tri, vbody, tex, texel, texn, {V->lc[0], V->lc[1], V->lc[2]}, {V->up[0], V->up[1], V->up[2]}};
    return s;
}

/* out u8[H][W][3]; tri_out (optional) int[H][W]: index of the triangle seen, -1 for the sky; depth_out (optional) double[H][W].
 * orc_vis_render_ex: ss = 1 | 2 samples per pixel and axis (2: the four samples at +-1/4 pixel of the centre are resolved and averaged; the
 * samples of a pixel that see the same triangle share the colour of the first of them -- MuJoCo's offscreen buffer is multisampled,
 * <quality offsamples> default 4 [EXT]); shadows != 0: a surface point that faces the scene's
 * directional light (scene.xml:48, castshadow default true [EXT]) and lies inside the light's shadow box (centre and half extent from
 * <statistic center extent>, scene.xml:6: render_light[7], [11], [15] and [3]) loses the light's diffuse term when another triangle lies
 * between it and the light -- one exact ray per sample where the device looks up a depth map rendered from the light.  tri_out /
 * depth_out hold the pixel-centre ray's answers. */
/* tnorm (orc_vis_render_sm; NULL = flat): per triangle the three corners' lighting normals in the body frame (compiler/vismesh.py corner_normals).  With
 * them every corner is lit with its own normal -- headlight term along the ray to the corner, the directional light's diffuse and specular terms, each
 * clamped as fixed-function GL clamps a vertex colour [EXT] -- and the three terms (shade, shade without the light's part, specular) are interpolated with
 * the hit point's barycentrics, which are perspective-correct by construction here. */
static int vis_render(const orc_data* d, int cam, int nvert, const double* vert, const int* vbody, int ntri, const int* tri, const double* rgb,
                      const double* uv, const int* tex, const int* texel, int texn, int H, int W, int ss, int shadows, const double* tnorm, unsigned char* out, int* tri_out, double* depth_out) {
    const orc_model* m = d->m;
    if (cam < 0 || cam >= m->ncam || !m->render_light || (ss != 1 && ss != 2)) return -1;
    vis_view V;
    if (vis_view_init(&V, d, cam, H, nvert, vert, vbody, ntri, tri)) return -2;
    const double *Rc = V.Rc, *pc = V.pc, *lw = V.lw, *e1 = V.e1, *e2 = V.e2, *vc = V.vc, *vw = V.vw, *L = m->render_light;
    const unsigned char* front = V.front;
    const double znear = V.znear, scale = V.scale;
    const double sh_half = shadows ? L[3] : 0.0, sh_s = V.sh_s, sh_t = V.sh_t;
    const vis_shader sh = vis_shader_of(&V, d, tri, vbody, rgb, uv, tex, texel, texn, tnorm);
    int hits = 0;
    const int ns = ss * ss;
    for (int i = 0; i < H; i++)
        for (int j = 0; j < W; j++) {
            double acc[3] = {0, 0, 0};
            int sid[4] = {-2, -2, -2, -2};            /* what the samples shaded so far saw (-1: the sky) and their quantised colours */
            double scol[4][3];
            for (int smp = -1; smp < ns; smp++) {
                /* smp = -1: the pixel centre (tri_out / depth_out; the colour too when ss = 1); 0 .. 3: the samples at +-1/4 pixel */
                if ((ss == 1) != (smp == -1)) { if (!(smp == -1 && (tri_out || depth_out))) continue; }
                const double ox = smp < 0 ? 0.0 : ((smp & 1) ? 0.25 : -0.25), oy = smp < 0 ? 0.0 : ((smp & 2) ? 0.25 : -0.25);
                const double dir[3] = {(j + 0.5 + ox - 0.5 * W) * scale, -(i + 0.5 + oy - 0.5 * H) * scale, -1.0};
                double best = 1e300, bu = 0, bv = 0;
                int bt = -1;
                for (int t = 0; t < ntri; t++) {
                    const double *a = vc + 3 * tri[3 * t], *bb = vc + 3 * tri[3 * t + 1], *c = vc + 3 * tri[3 * t + 2];
                    const double e1_[3] = {bb[0] - a[0], bb[1] - a[1], bb[2] - a[2]}, e2_[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
                    const double h[3] = {dir[1] * e2_[2] - dir[2] * e2_[1], dir[2] * e2_[0] - dir[0] * e2_[2], dir[0] * e2_[1] - dir[1] * e2_[0]};
                    const double det = e1_[0] * h[0] + e1_[1] * h[1] + e1_[2] * h[2];
                    if (fabs(det) < 1e-300) continue;
                    const double s_[3] = {-a[0], -a[1], -a[2]};
                    const double u = (s_[0] * h[0] + s_[1] * h[1] + s_[2] * h[2]) / det;
                    if (u < 0 || u > 1) continue;
                    const double q[3] = {s_[1] * e1_[2] - s_[2] * e1_[1], s_[2] * e1_[0] - s_[0] * e1_[2], s_[0] * e1_[1] - s_[1] * e1_[0]};
                    const double v = (dir[0] * q[0] + dir[1] * q[1] + dir[2] * q[2]) / det;
                    if (v < 0 || u + v > 1) continue;
                    const double tt = (e2_[0] * q[0] + e2_[1] * q[1] + e2_[2] * q[2]) / det;      /* = depth along the optical axis (dir z = -1) */
                    if (!front[t]) continue;                                                     /* back faces are culled (as MuJoCo's renderer does [EXT]) */
                    if (tt >= znear && tt < best) { best = tt; bt = t; bu = u; bv = v; }
                }
                if (smp == -1) {
                    if (tri_out) tri_out[(size_t)i * W + j] = bt;
                    if (depth_out) depth_out[(size_t)i * W + j] = bt >= 0 ? best : 0.0;
                    if (bt >= 0) hits++;
                    if (ss != 1) continue;
                }
                double col[3];
                /* a fragment -- the samples of the pixel that one triangle wins, or that see the sky -- is shaded once, at its first sample, as a
                 * multisampled GL buffer does [EXT]: a later sample of the same fragment takes that colour */
                int prev = -1;
                for (int s2 = 0; s2 < smp; s2++)
                    if (sid[s2] == bt && prev < 0) prev = s2;
                if (smp >= 0 && prev >= 0) {
                    sid[smp] = bt;
                    for (int k = 0; k < 3; k++) { scol[smp][k] = scol[prev][k]; acc[k] += scol[prev][k]; }
                    continue;
                }
                int shadowed = 0;
                if (bt >= 0) {
                    const double cl = vis_light_cos(&sh, bt);
                    if (cl > 0 && sh_half > 0) {
                        /* the sample's surface point in the world, a ray from it towards the light */
                        const double P[3] = {dir[0] * best, dir[1] * best, dir[2] * best};
                        double pw[3];
                        for (int k = 0; k < 3; k++) pw[k] = pc[k] + Rc[3 * k] * P[0] + Rc[3 * k + 1] * P[1] + Rc[3 * k + 2] * P[2];
                        const double ps = pw[0] * e1[0] + pw[1] * e1[1] + pw[2] * e1[2], pt = pw[0] * e2[0] + pw[1] * e2[1] + pw[2] * e2[2];
                        if (fabs(ps - sh_s) < sh_half && fabs(pt - sh_t) < sh_half) {
                            const double rd[3] = {-lw[0], -lw[1], -lw[2]};
                            for (int t = 0; t < ntri; t++) {
                                if (t == bt) continue;
                                const double *A = vw + 3 * tri[3 * t], *B = vw + 3 * tri[3 * t + 1], *C = vw + 3 * tri[3 * t + 2];
                                const double f1[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]}, f2[3] = {C[0] - A[0], C[1] - A[1], C[2] - A[2]};
                                const double h[3] = {rd[1] * f2[2] - rd[2] * f2[1], rd[2] * f2[0] - rd[0] * f2[2], rd[0] * f2[1] - rd[1] * f2[0]};
                                const double det = f1[0] * h[0] + f1[1] * h[1] + f1[2] * h[2];
                                if (fabs(det) < 1e-300) continue;
                                const double s_[3] = {pw[0] - A[0], pw[1] - A[1], pw[2] - A[2]};
                                const double u = (s_[0] * h[0] + s_[1] * h[1] + s_[2] * h[2]) / det;
                                if (u < 0 || u > 1) continue;
                                const double q[3] = {s_[1] * f1[2] - s_[2] * f1[1], s_[2] * f1[0] - s_[0] * f1[2], s_[0] * f1[1] - s_[1] * f1[0]};
                                const double v = (rd[0] * q[0] + rd[1] * q[1] + rd[2] * q[2]) / det;
                                if (v < 0 || u + v > 1) continue;
                                const double tt = (f2[0] * q[0] + f2[1] * q[1] + f2[2] * q[2]) / det;
                                if (tt > 1e-4) { shadowed = 1; break; }
                            }
                        }
                    }
                }
                vis_shade(&sh, bt, bu, bv, dir, shadowed, col);
                /* (the device shades a triangle once, in rgb8, and averages those: quantise before averaging) */
                for (int k = 0; k < 3; k++) {
                    const double qv = (double)vq8(col[k]);
                    acc[k] += qv;
                    if (smp >= 0) scol[smp][k] = qv;
                }
                if (smp >= 0) sid[smp] = bt;
            }
            for (int k = 0; k < 3; k++) out[((size_t)i * W + j) * 3 + k] = (unsigned char)(acc[k] / (ss == 1 ? 1 : ns) + 0.5);
        }
    vis_view_free(&V);
    return hits;
}

int orc_vis_render_ex(const orc_data* d, int cam, int nvert, const double* vert, const int* vbody, int ntri, const int* tri, const double* rgb,
                      const double* uv, const int* tex, const int* texel, int texn, int H, int W, int ss, int shadows, unsigned char* out, int* tri_out, double* depth_out) {
    return vis_render(d, cam, nvert, vert, vbody, ntri, tri, rgb, uv, tex, texel, texn, H, W, ss, shadows, NULL, out, tri_out, depth_out);
}

int orc_vis_render_sm(const orc_data* d, int cam, int nvert, const double* vert, const int* vbody, int ntri, const int* tri, const double* rgb,
                      const double* uv, const int* tex, const int* texel, int texn, const double* tnorm, int H, int W, int ss, int shadows, unsigned char* out, int* tri_out, double* depth_out) {
    return vis_render(d, cam, nvert, vert, vbody, ntri, tri, rgb, uv, tex, texel, texn, H, W, ss, shadows, tnorm, out, tri_out, depth_out);
}

int orc_vis_render(const orc_data* d, int cam, int nvert, const double* vert, const int* vbody, int ntri, const int* tri, const double* rgb,
                   const double* uv, const int* tex, const int* texel, int texn, int H, int W, unsigned char* out, int* tri_out, double* depth_out) {
    return orc_vis_render_ex(d, cam, nvert, vert, vbody, ntri, tri, rgb, uv, tex, texel, texn, H, W, 1, 0, out, tri_out, depth_out);
}

/* Which of the triangles that are DRAWN for triangle t holds the point with barycentrics (u of corner 1, v of corner 2): a triangle with one
 * corner nearer than znear is cut there (Sutherland-Hodgman in the corners' order: 0, 1, 2, with the crossing of an edge after the edge's
 * first corner) into a quadrilateral Q0 Q1 Q2 Q3 and drawn as the fan (Q0, Q1, Q2), (Q0, Q2, Q3): 0 or 1; every other triangle is drawn whole: 0. */
static int vis_drawn_part(const vis_shader* s, int t, double znear, double u, double v) {
    const double bc[3][2] = {{0, 0}, {1, 0}, {0, 1}};
    double D[3], Q[4][2];
    int nq = 0, nin = 0;
    for (int i = 0; i < 3; i++) { D[i] = -s->vc[3 * s->tri[3 * t + i] + 2]; nin += D[i] >= znear; }
    if (nin != 2) return 0;
    for (int i = 0; i < 3; i++) {
        const int j = i == 2 ? 0 : i + 1, in_i = D[i] >= znear, in_j = D[j] >= znear;
        if (in_i) { Q[nq][0] = bc[i][0]; Q[nq][1] = bc[i][1]; nq++; }
        if (in_i != in_j) {
            const double w = (znear - D[i]) / (D[j] - D[i]);
            Q[nq][0] = bc[i][0] + w * (bc[j][0] - bc[i][0]); Q[nq][1] = bc[i][1] + w * (bc[j][1] - bc[i][1]); nq++;
        }
    }
    const double dx = Q[2][0] - Q[0][0], dy = Q[2][1] - Q[0][1];
    const double side_p = dx * (v - Q[0][1]) - dy * (u - Q[0][0]), side_1 = dx * (Q[1][1] - Q[0][1]) - dy * (Q[1][0] - Q[0][0]);
    return (side_p >= 0) == (side_1 >= 0) ? 0 : 1;
}

/* ------------------------------------------------------------------------------------------------------------------------------------------
 * The f64 model of the device's depth-map shadow (DESIGN.md "The renderer's shadow contract").
 *
 * orc_vis_shadow_map: map[shn][shn], the largest height towards the light that a ray along the light through each texel's centre finds on
 * any triangle of the scene (front or back face, the receiver's own included), -INFINITY where it finds none.  Texel (x, y) covers
 * [x, x + 1) x [y, y + 1) texels of the light's box (s from sh_s - half, t from sh_t - half, shn / (2 half) texels per metre).  A triangle
 * is only tried on the texels inside its bounding box: no ray through another texel's centre can hit it. */
int orc_vis_shadow_map(const orc_data* d, int nvert, const double* vert, const int* vbody, int ntri, const int* tri, int shn, double* map) {
    const orc_model* m = d->m;
    if (!m->render_light || shn < 1) return -1;
    const double* L = m->render_light;
    const double ln = sqrt(L[4] * L[4] + L[5] * L[5] + L[6] * L[6]), lw[3] = {L[4] / ln, L[5] / ln, L[6] / ln}, half = L[3], itex = shn / (2.0 * half);
    double e1[3], e2[3];
    light_frame(lw, e1, e2);
    const double s0 = L[7] * e1[0] + L[11] * e1[1] + L[15] * e1[2] - half, t0 = L[7] * e2[0] + L[11] * e2[1] + L[15] * e2[2] - half;
    for (size_t k = 0; k < (size_t)shn * shn; k++) map[k] = -INFINITY;
    int filled = 0;
    for (int t = 0; t < ntri; t++) {
        double P[3][3];
        for (int c = 0; c < 3; c++) {
            const int v = tri[3 * t + c];
            const double *R = d->xmat + 9 * vbody[v], *p = d->xpos + 3 * vbody[v], *x = vert + 3 * v;
            double w[3];
            for (int i = 0; i < 3; i++) w[i] = R[3 * i] * x[0] + R[3 * i + 1] * x[1] + R[3 * i + 2] * x[2] + p[i];
            P[c][0] = (w[0] * e1[0] + w[1] * e1[1] + w[2] * e1[2] - s0) * itex;
            P[c][1] = (w[0] * e2[0] + w[1] * e2[1] + w[2] * e2[2] - t0) * itex;
            P[c][2] = -(w[0] * lw[0] + w[1] * lw[1] + w[2] * lw[2]);
        }
        const double area = (P[1][0] - P[0][0]) * (P[2][1] - P[0][1]) - (P[2][0] - P[0][0]) * (P[1][1] - P[0][1]);
        if (!(fabs(area) > 1e-300)) continue;          /* edge-on to the light: no ray along the light crosses it */
        const double xmin = fmin(P[0][0], fmin(P[1][0], P[2][0])), xmax = fmax(P[0][0], fmax(P[1][0], P[2][0]));
        const double ymin = fmin(P[0][1], fmin(P[1][1], P[2][1])), ymax = fmax(P[0][1], fmax(P[1][1], P[2][1]));
        if (xmax < 0 || ymax < 0 || xmin > shn || ymin > shn) continue;
        const int ix0 = (int)fmax(0.0, ceil(xmin - 0.5)), ix1 = (int)fmin(shn - 1.0, floor(xmax - 0.5));
        const int iy0 = (int)fmax(0.0, ceil(ymin - 0.5)), iy1 = (int)fmin(shn - 1.0, floor(ymax - 0.5));
        for (int y = iy0; y <= iy1; y++)
            for (int x = ix0; x <= ix1; x++) {
                const double fx = x + 0.5, fy = y + 0.5;
                const double l0 = ((P[1][0] - fx) * (P[2][1] - fy) - (P[2][0] - fx) * (P[1][1] - fy)) / area;
                const double l1 = ((P[2][0] - fx) * (P[0][1] - fy) - (P[0][0] - fx) * (P[2][1] - fy)) / area;
                const double l2 = 1.0 - l0 - l1;
                if (l0 < 0 || l1 < 0 || l2 < 0) continue;
                const double h = l0 * P[0][2] + l1 * P[1][2] + l2 * P[2][2];
                double* q = map + (size_t)y * shn + x;
                if (*q == -INFINITY) filled++;
                if (h > *q) *q = h;
            }
    }
    return filled;
}

/* orc_vis_render_model: the image of orc_vis_render_sm with ss = 1 | 2, every ray of the sampling pattern moved by (dx, dy) pixel, and the
 * shadow of the device's contract in place of the exact ray.  map: an orc_vis_shadow_map of shn texels a side (of this state, or of another
 * one for a counter-image; NULL: no shadows).  A sample whose triangle faces the light (flat normal, cosine cl > 0) and whose light-plane
 * coordinates (su, sv), in texels, lie in [0, shn)^2 is shadowed when the map's value at texel (floor su, floor sv) is not empty and exceeds
 * the sample's height towards the light by more than bias = bias_scale (1e-3 + 1.5 tan(theta) / itex), tan(theta) = sqrt(1 - cl^2) / max(cl, 0.05).
 *
 * The verdict of a sample is FRAGILE when a texel that holds a point within eps_tex texels of (su, sv) -- or the outside of the box, if that
 * is as near -- gives the other verdict, or when the map's value is within delta of height + bias.  A fragile fragment contributes its lit
 * colour to one of out_lo / out_hi and its shadowed colour to the other; everywhere else out_lo = out_hi = out.
 *
 * out, out_lo, out_hi: u8 [H][W][3].  Optional: dmin / dmax double [H][W], the smallest and largest depth of the pixel's samples (0: sky);
 * flag u8 [H][W], bit 0: a fragment of the pixel is shadowed, bit 1: one is fragile, bit 2: one was looked up in the map; bias_out double
 * [H][W], the largest bias of the pixel's fragments (0: none looked up); samp_tri int [H][W][ss ss], the triangle of every sample;
 * samp_flag u8 [H][W][ss ss], the bits above per sample (0 for a sample that took an earlier sample's colour).
 * The fragment rule: a fragment -- the samples of a pixel that one drawn triangle wins -- is shaded, and looked up, once, at its first sample.
 * The device draws a triangle that the near plane cuts into a quadrilateral as two triangles, each with fragments of its own (as GL
 * rasterises the triangles its clipper makes); orc_vis_render_sm, which never clips, takes the whole triangle as one. */
int orc_vis_render_model(const orc_data* d, int cam, int nvert, const double* vert, const int* vbody, int ntri, const int* tri, const double* rgb,
                         const double* uv, const int* tex, const int* texel, int texn, const double* tnorm, int H, int W, int ss, double dx, double dy,
                         int shn, const double* map, double bias_scale, double eps_tex, double delta, unsigned char* out, unsigned char* out_lo,
                         unsigned char* out_hi, double* dmin, double* dmax, unsigned char* flag, double* bias_out, int* samp_tri, unsigned char* samp_flag) {
    const orc_model* m = d->m;
    if (cam < 0 || cam >= m->ncam || !m->render_light || (ss != 1 && ss != 2) || (map && shn < 1)) return -1;
    vis_view V;
    if (vis_view_init(&V, d, cam, H, nvert, vert, vbody, ntri, tri)) return -2;
    const vis_shader sh = vis_shader_of(&V, d, tri, vbody, rgb, uv, tex, texel, texn, tnorm);
    const double *vc = V.vc, *L = m->render_light, half = L[3], itex = map ? shn / (2.0 * half) : 0.0;
    /* A ray that hits a triangle at depth >= znear passes through the part of the triangle at that depth or beyond, so its direction (x / depth,
     * y / depth) lies in the bounding box of that part's corners: the box only spares the exact test below where it cannot succeed.  Back
     * faces are left out as vis_render leaves them out. */
    int nf = 0;
    int* fl = (int*)malloc(sizeof(int) * ((size_t)ntri + 1));
    double* box = (double*)malloc(sizeof(double) * 4 * ((size_t)ntri + 1));
    if (!fl || !box) { free(fl); free(box); vis_view_free(&V); return -2; }
    for (int t = 0; t < ntri; t++) {
        if (!V.front[t]) continue;
        double* b = box + 4 * nf;
        b[0] = b[2] = 1e300; b[1] = b[3] = -1e300;
        const double zc = V.znear * (1.0 - 1e-9);           /* a hit counts from depth znear on: the part of the triangle at depth >= zc */
        for (int c = 0; c < 3; c++) {
            const double *p = vc + 3 * tri[3 * t + c], *q = vc + 3 * tri[3 * t + (c + 1) % 3];
            double pts[2][3];
            int np_ = 0;
            if (-p[2] >= zc) { pts[np_][0] = p[0]; pts[np_][1] = p[1]; pts[np_][2] = p[2]; np_++; }
            if ((-p[2] >= zc) != (-q[2] >= zc)) {            /* the edge crosses the plane */
                const double w = (zc + p[2]) / (p[2] - q[2]);
                pts[np_][0] = p[0] + w * (q[0] - p[0]); pts[np_][1] = p[1] + w * (q[1] - p[1]); pts[np_][2] = -zc; np_++;
            }
            for (int k = 0; k < np_; k++) {
                const double x = pts[k][0] / -pts[k][2], y = pts[k][1] / -pts[k][2], mg = 1e-9 * (1.0 + fabs(x) + fabs(y));
                b[0] = fmin(b[0], x - mg); b[1] = fmax(b[1], x + mg); b[2] = fmin(b[2], y - mg); b[3] = fmax(b[3], y + mg);
            }
        }
        if (b[0] > b[1]) continue;                          /* wholly nearer than the near plane */
        fl[nf++] = t;
    }
    int hits = 0;
    const int ns = ss * ss;
    int* rowl = (int*)malloc(sizeof(int) * ((size_t)nf + 1));        /* the boxes that reach into the image row's band of sample rays */
    if (!rowl) { free(fl); free(box); vis_view_free(&V); return -2; }
    for (int i = 0; i < H; i++) {
        const double yt = -(i + 0.5 - 0.25 + dy - 0.5 * H) * V.scale, yb = -(i + 0.5 + 0.25 + dy - 0.5 * H) * V.scale;
        int nr = 0;
        for (int f = 0; f < nf; f++)
            if (box[4 * f + 2] <= yt && box[4 * f + 3] >= yb) rowl[nr++] = f;
        for (int j = 0; j < W; j++) {
            const size_t px = (size_t)i * W + j;
            double acc[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};        /* the nominal image, the lower and the upper one */
            int sid[4] = {-2, -2, -2, -2};
            double scol[4][3][3], lo_d = 1e300, hi_d = 0.0, pbias = 0.0;
            unsigned pflag = 0;
            for (int smp = 0; smp < ns; smp++) {
                const double ox = ss == 1 ? 0.0 : ((smp & 1) ? 0.25 : -0.25), oy = ss == 1 ? 0.0 : ((smp & 2) ? 0.25 : -0.25);
                const double dir[3] = {(j + 0.5 + ox + dx - 0.5 * W) * V.scale, -(i + 0.5 + oy + dy - 0.5 * H) * V.scale, -1.0};
                double best = 1e300, bu = 0, bv = 0;
                int bt = -1;
                for (int r = 0; r < nr; r++) {
                    const int f = rowl[r];
                    const double* b = box + 4 * f;
                    if (dir[0] < b[0] || dir[0] > b[1] || dir[1] < b[2] || dir[1] > b[3]) continue;
                    const int t = fl[f];
                    const double *a = vc + 3 * tri[3 * t], *bb = vc + 3 * tri[3 * t + 1], *c = vc + 3 * tri[3 * t + 2];
                    const double e1_[3] = {bb[0] - a[0], bb[1] - a[1], bb[2] - a[2]}, e2_[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
                    const double h[3] = {dir[1] * e2_[2] - dir[2] * e2_[1], dir[2] * e2_[0] - dir[0] * e2_[2], dir[0] * e2_[1] - dir[1] * e2_[0]};
                    const double det = e1_[0] * h[0] + e1_[1] * h[1] + e1_[2] * h[2];
                    if (fabs(det) < 1e-300) continue;
                    const double s_[3] = {-a[0], -a[1], -a[2]};
                    const double u = (s_[0] * h[0] + s_[1] * h[1] + s_[2] * h[2]) / det;
                    if (u < 0 || u > 1) continue;
                    const double q[3] = {s_[1] * e1_[2] - s_[2] * e1_[1], s_[2] * e1_[0] - s_[0] * e1_[2], s_[0] * e1_[1] - s_[1] * e1_[0]};
                    const double v = (dir[0] * q[0] + dir[1] * q[1] + dir[2] * q[2]) / det;
                    if (v < 0 || u + v > 1) continue;
                    const double tt = (e2_[0] * q[0] + e2_[1] * q[1] + e2_[2] * q[2]) / det;
                    if (tt >= V.znear && tt < best) { best = tt; bt = t; bu = u; bv = v; }
                }
                if (bt >= 0) hits++;
                const double dep = bt >= 0 ? best : 0.0;
                lo_d = fmin(lo_d, dep); hi_d = fmax(hi_d, dep);
                if (samp_tri) samp_tri[px * ns + smp] = bt;
                if (samp_flag) samp_flag[px * ns + smp] = 0;
                /* a fragment: the samples of the pixel that one DRAWN triangle wins (vis_drawn_part), or that see the sky */
                const int fid = bt < 0 ? -1 : 2 * bt + vis_drawn_part(&sh, bt, V.znear, bu, bv);
                int prev = -1;
                for (int s2 = 0; s2 < smp; s2++)
                    if (sid[s2] == fid && prev < 0) prev = s2;
                sid[smp] = fid;
                if (prev >= 0) {
                    for (int w = 0; w < 3; w++)
                        for (int k = 0; k < 3; k++) { scol[smp][w][k] = scol[prev][w][k]; acc[w][k] += scol[prev][w][k]; }
                    continue;
                }
                int shadowed = 0, fragile = 0, looked = 0;
                if (bt >= 0 && map) {
                    const double cl = vis_light_cos(&sh, bt);
                    if (cl > 0) {
                        const double P[3] = {dir[0] * best, dir[1] * best, dir[2] * best};
                        double pw[3];
                        for (int k = 0; k < 3; k++) pw[k] = V.pc[k] + V.Rc[3 * k] * P[0] + V.Rc[3 * k + 1] * P[1] + V.Rc[3 * k + 2] * P[2];
                        const double su = (pw[0] * V.e1[0] + pw[1] * V.e1[1] + pw[2] * V.e1[2] - (V.sh_s - half)) * itex;
                        const double sv = (pw[0] * V.e2[0] + pw[1] * V.e2[1] + pw[2] * V.e2[2] - (V.sh_t - half)) * itex;
                        const double hh = -(pw[0] * V.lw[0] + pw[1] * V.lw[1] + pw[2] * V.lw[2]);
                        const double bias = bias_scale * (1e-3 + 1.5 * sqrt(fmax(0.0, 1.0 - cl * cl)) / fmax(cl, 0.05) / itex);
                        looked = 1;
                        if (bias > pbias) pbias = bias;
                        /* the verdict at (su, sv), then at the texels (or the outside) within eps_tex of it */
                        for (int pass = 0; pass < 2; pass++) {
                            const double r = pass ? eps_tex : 0.0;
                            for (double y = floor(sv - r); y <= floor(sv + r); y += 1.0)
                                for (double x = floor(su - r); x <= floor(su + r); x += 1.0) {
                                    int v = 0;
                                    if (x >= 0 && y >= 0 && x < shn && y < shn) {
                                        const double mh = map[(size_t)y * shn + (size_t)x];
                                        v = mh != -INFINITY && mh > hh + bias;
                                        if (mh != -INFINITY && fabs(mh - (hh + bias)) < delta) fragile = 1;
                                    }
                                    if (!pass) shadowed = v;
                                    else if (v != shadowed) fragile = 1;
                                }
                        }
                    }
                }
                double col[2][3];
                vis_shade(&sh, bt, bu, bv, dir, shadowed, col[0]);
                if (fragile) vis_shade(&sh, bt, bu, bv, dir, !shadowed, col[1]);
                for (int k = 0; k < 3; k++) {
                    const double q0 = (double)vq8(col[0][k]), q1 = fragile ? (double)vq8(col[1][k]) : q0;
                    scol[smp][0][k] = q0; scol[smp][1][k] = fmin(q0, q1); scol[smp][2][k] = fmax(q0, q1);
                    for (int w = 0; w < 3; w++) acc[w][k] += scol[smp][w][k];
                }
                const unsigned fb = (shadowed ? 1u : 0u) | (fragile ? 2u : 0u) | (looked ? 4u : 0u);
                pflag |= fb;
                if (samp_flag) samp_flag[px * ns + smp] = (unsigned char)fb;
            }
            for (int k = 0; k < 3; k++) {
                out[px * 3 + k] = (unsigned char)(acc[0][k] / ns + 0.5);
                out_lo[px * 3 + k] = (unsigned char)(acc[1][k] / ns + 0.5);
                out_hi[px * 3 + k] = (unsigned char)(acc[2][k] / ns + 0.5);
            }
            if (dmin) dmin[px] = lo_d;
            if (dmax) dmax[px] = hi_d;
            if (flag) flag[px] = (unsigned char)pflag;
            if (bias_out) bias_out[px] = pbias;
        }
    }
    free(rowl);
    free(fl);
    free(box);
    vis_view_free(&V);
    return hits;
}
