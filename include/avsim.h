/* include/avsim.h -- C-ABI of libavsim.so: the MI355X-native batched replacement for the hot path
 * of the AV-ALOHA gym_guided_vision environments.
 *
 * Boundary it replaces (reference file:line, all under /root/reference):
 *   gym_guided_vision/gym_guided_vision/env.py:36-166   GuidedVisionEnv.__init__  -> avsim_create
 *   env.py:228-249 (+ task overrides :474-501,:513-543,:604-637,:705-735,:792-818) reset -> avsim_reset
 *   env.py:203-226 step / :255-269 step_action (20 x MuJoCo mj_step, env.py:218)   -> avsim_step
 *   env.py:168-178 get_obs agent_pos, :425-863 get_reward x5, :224 is_success       -> outputs of avsim_step
 *   env.py:251-253 set_qpos                                                          -> avsim_set_qpos
 *   data_collection_scripts/sim_env.py:277-312 step with IK (GradIK/DiffIK)          -> avsim_step_cartesian
 *   data_collection_scripts/diff_ik.py:89-90 DiffIK.run, grad_ik.py:150-166 GradIK.run -> avsim_ik
 *
 * Conventions: every entry point returns 0 on success or a negative AVSIM_E* code; the message is
 * available from avsim_last_error().  All bulk pointers are HOST pointers unless the handle was
 * created with AVSIM_IO_DEVICE, in which case they are device pointers on the handle's device and
 * work is enqueued on the handle's stream without synchronising (call avsim_sync).  The library
 * never keeps a caller pointer past the call.  One host thread per handle; handles are independent.
 * There is NO CPU fallback: creation fails if no gfx950 device is usable.
 */
#ifndef AVSIM_H
#define AVSIM_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct avsim avsim_t;

enum {
    AVSIM_OK = 0,
    AVSIM_EINVAL = -1,  /* bad argument (python facade: AssertionError / ValueError) */
    AVSIM_ENODEV = -2,  /* no usable HIP device */
    AVSIM_EHIP = -3,    /* HIP runtime error, text in avsim_last_error */
    AVSIM_EMODEL = -4,  /* malformed model blob */
    AVSIM_ENOTIMPL = -5 /* python facade: NotImplementedError (env.py:30) */
};

enum {
    AVSIM_IO_DEVICE = 1u << 0, /* bulk I/O pointers are device pointers */
    AVSIM_F64_PHYSICS = 1u << 1 /* debug: run the physics kernels in double precision */
};

/* IK controller selection for avsim_step_cartesian / avsim_ik */
enum {
    AVSIM_IK_REFERENCE = 0, /* left/right GradIK, middle DiffIK (sim_env.py:89-138) */
    AVSIM_IK_DLS = 1        /* damped least squares on all three arms (BASELINE.json north_star) */
};

/* dims[]: 0 nq, 1 nv, 2 nu (actuators, 21), 3 num_joints of the action/agent_pos (14|21), 4 nobj (free objects),
 * 5 max_reward, 6 num_envs, 7 task id, 8 ncon capacity, 9 nefc capacity (the full tier), 10 LDS bytes per block (one env per
 * wavefront with the first tier's record + the hot model tables), 11 blocks that fit one CU's 160 KiB */
#define AVSIM_NDIMS 12

/* Build a batched simulation from a compiled model blob (av_aloha_amd/compiler, replaces env.py:53-56).
 * num_arms is encoded in the blob (2-arm blobs carry the hidden middle arm of env.py:394-395). */
int avsim_create(const void* model_blob, size_t nbytes, int num_envs, int device, uint32_t flags, avsim_t** out);
void avsim_destroy(avsim_t* h);
const char* avsim_last_error(const avsim_t* h); /* h may be NULL for creation errors */
int avsim_dims(const avsim_t* h, int32_t dims[AVSIM_NDIMS]);

/* Solver / capacity / debug knobs (returns AVSIM_EINVAL for an unknown name or a value out of range):
 *   "solver"            0 PGS (BASELINE north_star), 1 Newton (MuJoCo's default, what the reference runs; default)
 *   "pgs_iters"         Gauss-Seidel sweeps of the PGS solver (default 20); "newton_iters" cap (default 100 = MuJoCo), "newton_tol" (1e-8 in f64 = MuJoCo, 1e-6 in f32)
 *   "ls_tolerance", "ls_iterations"   Newton's exact line search: stop when |phi'(alpha)| < ls_tolerance x |phi'(0)|, at most ls_iterations evaluations
 *                       after the one at alpha = 0.  Defaults 1e-10 (f64) / 1e-4 (f32) and 50.  MuJoCo's mjOption.ls_iterations is 50 and its
 *                       ls_tolerance 0.01, applied to a differently scaled derivative [EXT]: the default here searches much further than MuJoCo
 *                       does (the whole-episode parity tests need both sides to take the same step to rounding) -- a listed deviation, DESIGN.md 2
 *   "maxefc", "maxcon"  constraint rows / contacts an env can hold (per-task defaults 176-480 / 48-96): the stride of the contact export
 *                       and of the global row scratch; setting one makes it the capacity of a single tier (one pass)
 *   "maxefc_first", "maxcon_first"   the FIRST tier of the two-tier capacities (defaults: SewNeedle 224 / 56 of 336 / 72, TubeTransfer
 *                       288 / 64 of 480 / 96; the other tasks have one tier): a launch steps every env with the LDS record of the first
 *                       tier -- more envs per CU --, and an env that needs more in some substep is stepped again from its untouched
 *                       state with the full capacities: by its wave in the two adjacent records of a wave pair ("pair_waves" 1, the
 *                       default, when the full record fits two small ones), else by a second pass over the list of such envs.
 *                       Results are those of one pass with the full capacities, bit for bit
 *   "qcqp_tridiag"      multiplier iteration of a sliding contact's noslip QCQP: 0 MuJoCo's Cholesky per iterate (f64 default), 1 the
 *                       same iterates on the Householder-tridiagonal form of the friction block, 2 tridiagonal form + secular-equation
 *                       steps (Newton on 1/r - 1/|y|; f32 default): the same multiplier within the iteration's own thresholds
 *   "num_joints"        14 | 21: width of the action / agent_pos rows, whatever the blob's arm count (a 3-arm env whose camera
 *                       arm was parked by hide_middle_arm, env.py:394-395, keeps its 21-D action on the 2-arm model)
 *   "waves_per_block"   envs per workgroup, 0 = as many as fit in 160 KiB of LDS (<= 8)
 *   "phys_specialised"  1 (default): a one-pass f32 launch takes the physics kernel compiled for the handle's model (LDS layout, table
 *                       offsets, dims and the default solver configuration as compile-time constants; csrc/avsim_phys_specs.h lists the
 *                       models and the values) when the handle's layout, table offsets, dims and integer solver options ("solver",
 *                       "newton_iters", "noslip_iters", "noslip_trees", "noslip_per_tree", "qcqp_tridiag", "newton_early_exit",
 *                       "newton_component", "ls_iterations", "num_joints") equal that kernel's exactly at the launch, the generic kernel
 *                       otherwise; 0 = always the generic kernel; 2 = require: a step whose launch would take the generic kernel (another
 *                       model, capacities changed by "maxefc" / "maxcon", one of those options off its default, f64, two capacity tiers)
 *                       fails with AVSIM_EINVAL before anything is enqueued -- avsim_step*,
 *                       avsim_reset, avsim_set_state / avsim_set_qpos and avsim_observe ask before their IK / reset / conversion kernels.
 *                       Same results to the last bit in all three settings
 *   "rows_paired"       1 (default): the contact rows of a substep are filled two per lane -- the translational and the rotational row along
 *                       one axis of a contact's frame -- whenever that takes fewer trips of the wave than one row per lane (12 contacts of
 *                       6 rows: one trip instead of two); 0 = always one row per lane, and the generic kernel (the per-model kernels pair
 *                       unconditionally: "phys_specialised" 2 refuses).  Same results to the last bit
 *   "noslip_iters"      0 .. 100: sweeps of the noslip pass after the solver (default: the model's own, 3 in the committed models)
 *   "noslip_per_tree"   1 (default): the dry-friction rows of the noslip pass are relaxed per kinematic tree, all trees at once
 *                       (models with <= 8 trees); 0 = six rows at a time through the Gauss-Seidel groups (what models with more
 *                       trees get); same results to rounding
 *   "noslip_trees"      1 (default): a noslip pass whose contacts all touch one kinematic tree runs per tree, octet t of the wave on tree t,
 *                       the trees' contact chains side by side; 0 = always the wave-wide Gauss-Seidel groups (same results to rounding)
 *   "newton_component"  1 (default): in a scene where some contact couples two kinematic trees (a needle in a gripper) Newton's dense
 *                       factorisation and substitutions run over the dofs of the coupled trees only, the other trees in their lane
 *                       octets; 0 = over all nv columns (the same bits: the entries in between are zeros)
 *   "newton_early_exit" 1 (default): when a Newton step ends in the active set it started from and no contact of either end is in the cone's
 *                       middle zone, the cost was one quadratic along the step and the point is its minimiser: the solver returns without
 *                       evaluating the gradient that would confirm it (a third of an iteration; same qacc, same forces); 0 = always evaluate
 *   "order_envs"        1 (default): workgroups take the envs in the order of their cost in the previous step, most expensive
 *                       first (results do not depend on it); 0 = in index order
 *   "export_contacts"   0 skips the per-step contact export (avsim_get_contacts); "kernel_timing" 1 brackets every physics
 *                       launch AND every image kernel of avsim_render_depth / avsim_render_labels / the proxy mode of avsim_render_rgb with HIP events
 *                       (avsim_kernel_time, avsim_render_kernel_time; at most 1024 event pairs are kept per list, older ones are folded
 *                       into a running sum); "profile_phases" 1 enables avsim_get_phase_cycles */
int avsim_set_option(avsim_t* h, const char* name, double value);

/* env.py:228-249 + task reset: envs with mask[i]!=0 (NULL = all) go to the home pose, zero velocity,
 * home ctrl; their free objects get obj_qpos[i][nobj][7] = [x y z qw qx qy qz]. Derived quantities are
 * refreshed (mj_forward).  mask: uint8[N]; obj_qpos: double[N][nobj*7]. */
int avsim_reset(avsim_t* h, const uint8_t* mask, const double* obj_qpos);

/* env.py:203-226: action float[N][num_joints] -> ctrl, nsub physics substeps, then
 * agent_pos double[N][num_joints], reward int32[N], success uint8[N]. Any output may be NULL. */
int avsim_step(avsim_t* h, const float* action, int nsub, double* agent_pos, int32_t* reward, uint8_t* success);

/* `physics.step(nstep)` with the control vector as it stands (env.py:218 after env.py:203-215 has written physics.data.ctrl; dm_control's
 * Physics.step): nsub substeps driven by the handle's ctrl -- what avsim_set_state / an earlier step left there --, outputs as avsim_step.
 * A replay of recorded actuator commands and substep-by-substep debugging go through this. */
int avsim_step_ctrl(avsim_t* h, int nsub, double* agent_pos, int32_t* reward, uint8_t* success);

/* sim_env.py:277-312: action double[N][23] Cartesian targets; IK on measured qpos -> ctrl; physics.
 * Outputs as avsim_step (agent_pos has 21 entries per env here). */
int avsim_step_cartesian(avsim_t* h, const double* action23, int ik_mode, int nsub, double* agent_pos,
                         int32_t* reward, uint8_t* success);

/* Stand-alone batched IK (diff_ik.py / grad_ik.py `run`): arm 0 left, 1 right, 2 middle;
 * q double[n][nj], pos double[n][3], quat_wxyz double[n][4] -> q_out double[n][nj] (nj = 6,6,7).
 * controller: 0 DiffIK, 1 GradIK; max_iters <= 0 keeps the reference's iteration count (10 / 50). */
int avsim_ik(avsim_t* h, int arm, int controller, int max_iters, int n, const double* q, const double* pos,
             const double* quat_wxyz, double* q_out);
/* kinematics.py:17-24 / :35-50 batched: T double[n][16], J double[n][6][nj] (either may be NULL) */
int avsim_fk_jac(avsim_t* h, int arm, int n, const double* q, double* T, double* J);

/* env.py:168-178 get_obs (agent_pos) and env.py get_reward / :224 is_success of the CURRENT state, no time
 * stepping; any output may be NULL.  Evaluating the reward advances SewNeedle's latch as env.py:686-689 does. */
int avsim_observe(avsim_t* h, double* agent_pos, int32_t* reward, uint8_t* success);

/* env.py:251-253 set_qpos (all envs, double[N][nq]) followed by forward kinematics + collision */
int avsim_set_qpos(avsim_t* h, const double* qpos);
/* full state for checkpoint / tests: qpos[N][nq], qvel[N][nv], ctrl[N][nu], warmstart[N][nv]; NULL = skip */
int avsim_get_state(avsim_t* h, double* qpos, double* qvel, double* ctrl, double* warmstart);
int avsim_set_state(avsim_t* h, const double* qpos, const double* qvel, const double* ctrl, const double* warmstart);
/* the object poses an env whose state diverged is put back to (what avsim_reset was given; the model's default poses before the
 * first reset): double[N][nobj][7].  Not touched by avsim_set_state / avsim_set_qpos -- a handle that continues another handle's
 * episode carries them over with this pair, next to avsim_get_latch / avsim_set_latch */
int avsim_get_reset_poses(avsim_t* h, double* obj_qpos);
int avsim_set_reset_poses(avsim_t* h, const double* obj_qpos);
/* the per-env reward latch int32[N] (SewNeedle's _threaded_needle, env.py:602, :631, :673, :686-689; 0 for the other tasks): part
 * of an env's state next to qpos / qvel / ctrl -- a checkpoint or a move of the env to another handle carries it along */
int avsim_get_latch(avsim_t* h, int32_t* latch);
int avsim_set_latch(avsim_t* h, const int32_t* latch);
/* contacts of the current state, env.py:436-441 view: ncon int32[N], geom pairs int32[N][cap][2], dist double[N][cap] */
int avsim_get_contacts(avsim_t* h, int32_t* ncon, int32_t* geom_pairs, double* dist);
/* per-env diagnostics of the last step: int32[N][4] = {ncon, nefc, overflow flags, packed}; packed = divergence flag (bit 0: the state became NaN / Inf / > 1e6 during the step and the env was put back to the
 * state its episode started from -- home pose, the objects where the last avsim_reset put them, zero velocity --, as MuJoCo resets
 * its data on a bad state) |
 * broad-phase survivors (bits 8-15) | Newton iterations summed over the substeps (bits 16-27) | their maximum, saturated at 15 (bits 28-31) */
int avsim_get_diag(avsim_t* h, int32_t* diag);

/* debug: shader-clock cycles each env's wave spent in the 8 phases (kinematics, CRB, RNE, smooth, collide, rows,
 * solve, integrate, + broad / narrow phase incl. the trailing refresh) during the last launch; needs
 * avsim_set_option("profile_phases", 1); int64[N][26]: 8 phases, broad, narrow, then the Newton solver's
 * init / gradient / Hessian / factorisation / line search / final forces / noslip / back-substitution cycles and 8 probe slots
 * (noslip: group steps, dry-friction passes, their cycles, look-ahead set-up, entry set-up, whole call; two free) */
int avsim_get_phase_cycles(avsim_t* h, int64_t* out);

/* Replaces the camera part of get_obs / render (gym_guided_vision/gym_guided_vision/env.py:180-188, :195-200; MuJoCo OpenGL
 * renderer) by depth images (BASELINE config 5): out = float32[N][ncam][height][width], metres along the optical axis of
 * camera cam_ids[c] (index into the model's camera table, manifest "camera_names"; avsim_camera_count entries), row 0 = top,
 * pixels that see nothing = far plane (30 m).  Drawn are the collision proxies of the current state.  `out` is a host or a
 * device pointer according to AVSIM_IO_DEVICE; cam_ids is always a host pointer.  Batches of more than 4096 envs (option "render_chunk")
 * go through the kernels in chunks, so that the per-view scratch (~100 KB) is bounded by the chunk. */
int avsim_render_depth(avsim_t* h, const int32_t* cam_ids, int ncam, int height, int width, float* out);

/* The same cameras as colour images, the layout of the reference's "pixels" observation and of render()
 * (env.py:180-188, :195-200): out = uint8[N][ncam][height][width][3] (RGB).  Once avsim_load_visual has run (the Python facades
 * do that on first use) the VISUAL scene is rasterised: the decimated visual meshes of the robots, the frame and camera mounts,
 * the textured table, the task objects (k_vis_render; flat Lambert shading under the scene's headlight scene.xml:9 and directional
 * light :48, table texture, skybox gradient :34).  Without a loaded visual scene, or with option "render_proxies" 1, the collision
 * proxies are drawn in their flat material colours instead (the depth rasteriser's colour variant).  Options of the visual image (round 5):
 * "render_shadows" 1 -- the scene's directional light (scene.xml:48) casts shadows inside its shadow box (<statistic center extent>,
 * scene.xml:6), from a 512 x 512 depth map rendered from the light per env ("render_shadow_size" 1024 | 2048: a finer one, 4 / 16 MB per env); "render_samples" 4 -- 2 x 2 supersampling (MuJoCo's offscreen
 * buffer is multisampled, offsamples default 4 [EXT]).  Both are off at the C-ABI and on in the gym facades.  "render_cam_major" 1 -- out is
 * uint8[ncam][N][height][width][3] (every camera's batch contiguous: the facades hand out one array per camera without copying).  The directional light's specular
 * term (MJCF defaults: light 0.3 x material 0.5, exponent 64) is part of the shade.  "render_smooth" 1 (round 6; on in the gym / Cartesian facades, off
 * at the C-ABI) -- the three corners of a triangle are lit with their own normals (the library's lib_tnorm: area-weighted means over the faces
 * within the crease angle, as MuJoCo generates vertex normals with smoothnormal="false" [EXT]) and the shade is interpolated perspective-correctly
 * over the triangle, as fixed-function GL lights per vertex; 0: one shade per triangle.  No transparency: a stand-in for MuJoCo's OpenGL output,
 * not a pixel match.  A view that runs out of triangle
 * records or tile-list entries sets the overflow flags of avsim_visual_info (the image then lacks triangles).  Pointer conventions
 * as avsim_render_depth. */
int avsim_render_rgb(avsim_t* h, const int32_t* cam_ids, int ncam, int height, int width, uint8_t* out);
/* The visual scene of avsim_render_rgb (env.py:180-188, :195-200 draw the visual meshes of aloha_sim.xml class
 * "visual", the frame and the textured table of scene.xml, the task objects): library_blob = models/visual_meshes.avv, the decimated
 * mesh library of av_aloha_amd/compiler/vismesh.py; the model blob given to avsim_create carries the instances (vis_inst_*).  After
 * it avsim_render_rgb rasterises those triangles (flat Lambert shading, table texture) instead of the collision proxies; option
 * "render_proxies" 1 switches back.  AVSIM_EMODEL when the model was compiled without instances or the library lacks a mesh. */
int avsim_load_visual(avsim_t* h, const void* library_blob, size_t nbytes);
/* info = {triangles, vertices of the loaded visual scene (0: none), overflow flags of the last visual render (bit 0: a view ran out
 * of triangle records, bit 1: of tile-list entries), instances in the model blob}; synchronises the stream */
int avsim_visual_info(avsim_t* h, int32_t info[4]);
/* debug: per-view records of the last visual render, int32[nviews][8] = {overflow bits, shader-clock cycles / 1024 of the stages
 * (vertex transform, triangle set-up, tile count, tile fill, tiles), triangle records, tile-list entries} */
int avsim_visual_profile(avsim_t* h, int32_t* out, int nviews);
int avsim_camera_count(const avsim_t* h);

/* avsim_render_rgb's visual-scene image as a policy reads it (eval.py:23-66 preprocess_observation: u8 HWC -> float32 CHW / 255):
 * out = float32[N][ncam][3][height][width] ([ncam][N][3][height][width] under "render_cam_major"), every value (float)u8 / 255 of the
 * u8 image of the same call, bit for bit.  Needs the visual scene (avsim_load_visual, render_proxies 0).  Pointer conventions as
 * avsim_render_depth; in device mode nothing synchronises once a call with the same cameras has run. */
int avsim_render_rgb_f32(avsim_t* h, const int32_t* cam_ids, int ncam, int height, int width, float* out);

/* What every pixel of avsim_render_depth's image shows (k_render_depth's labels mode); av_aloha_amd/segment.py is the
 * specification and holds the tables.  The same cast of the same collision proxies, with the winning geom kept: labels =
 * uint8[N][ncam][height][width], table[g] of the geom g the pixel sees (g indexes the model's collision geom table, manifest "geom_names"),
 * table[ngeom] where it sees nothing.  table NULL is the identity, table[g] = g, with 255 for nothing.  depth = float32 of the same shape:
 * where the pixel's label is not dropped, avsim_render_depth's image of the same state, cameras and size BIT FOR BIT; where drop[label] != 0,
 * the far plane (30 m), the value of a ray that hits nothing -- so that avsim_point_cloud, avsim_voxel_grid and avsim_virtual_views, which
 * keep d < max_depth, leave those pixels out (the robot leaves a cloud this way).  labels always holds the true label, dropped or not.
 * Either output may be NULL, not both.  depth and labels follow the handle's I/O mode; with AVSIM_IO_DEVICE and a width that is a multiple
 * of 4, depth is 16-byte and labels 4-byte aligned (a row's four pixels leave in one store).  cam_ids, table (ngeom + 1 entries) and drop
 * (256 flags) are HOST arrays in both modes, copied before the call returns.  The body poses are refreshed when they are another state's,
 * as the render calls do; the envs go through the kernels in the chunks of option "render_chunk".  With AVSIM_IO_DEVICE nothing
 * synchronises once a call of the same size has run.  Invisible geoms (the pin spheres) are never drawn; their table entries are unused.
 * AVSIM_EINVAL, with nothing launched and the outputs untouched: ncam outside 1..16, height or width outside 1..4096, a camera id out of
 * range, a null cam_ids, depth and labels both NULL, drop given with depth NULL, a misaligned device pointer (above).
 * Debug option "render_labels_form" 1 keeps a lane's eight winners in eight registers instead of two: the same images, there so that
 * tools/bench_segment.py can time both in one process. */
int avsim_render_labels(avsim_t* h, const int32_t* cam_ids, int ncam, int height, int width,
                        const uint8_t* table /* host [ngeom + 1] or NULL */, const uint8_t* drop /* host [256] or NULL */,
                        float* depth /* [N][ncam][H][W] or NULL */, uint8_t* labels /* [N][ncam][H][W] or NULL */);

/* Point clouds from depth images on the device (csrc/avsim_pointcloud.hip); av_aloha_amd/pointcloud.py is the specification.
 * avsim_camera_poses: out = float32[N][ncam][16], the world pose of camera cam_ids[c] in every env at the CURRENT state -- position pc[3],
 * rotation Rc[9] (row major, camera frame to world; the camera looks along its -z, x to the right, y up), tan(fovy / 2) as the device's
 * table holds it, three zeros.  From the body pose (pb, Rb) and the model's camera offset (cp, Rm) in float32, every product and sum rounded
 * on its own, left to right: Rc[i][j] = (Rb[i][0] Rm[0][j] + Rb[i][1] Rm[1][j]) + Rb[i][2] Rm[2][j], pc[i] = ((pb[i] + Rb[i][0] cp[0]) +
 * Rb[i][1] cp[1]) + Rb[i][2] cp[2].  The body poses are refreshed when they are another state's, as the render calls do.  `out` follows the
 * handle's I/O mode, cam_ids is a host array.  AVSIM_EINVAL: ncam outside 1..16, a camera id out of range, a null pointer.
 *
 * avsim_point_cloud: one fixed-size cloud per env in the world frame, from ncam depth images [N][ncam][height][width] as avsim_render_depth
 * writes them.  The caller supplies the depth -- normally the tensor just rendered for the same state and cameras --, THE POSES ARE THOSE OF
 * THE CURRENT STATE (the records avsim_camera_poses returns, computed by the same kernel): a depth image of an earlier state is deprojected
 * with the wrong extrinsics.  All arithmetic is float32, every operation rounded on its own, and the result equals the specification bit
 * for bit given the pose records.
 *   Deprojection: with t = tan(fovy / 2), scale = 2 t / (float)H; pixel (r, c) has x = ((c + 0.5) - 0.5 W) scale, y = -(((r + 0.5) - 0.5 H)
 *     scale) -- the renderer's own rays --, the camera-frame point is (x d, y d, -d) and w[i] = ((pc[i] + Rc[i][0] X) + Rc[i][1] Y) +
 *     Rc[i][2] Z.
 *   Crop: a pixel is a candidate when d < max_depth and bounds lo[i] <= w[i] <= hi[i] on the three axes (inclusive; a NaN anywhere drops
 *     the pixel).  The candidates of an env are ordered by (camera slot, row, column); M is their number.
 *   Cap: AVSIM_PC_MAX_CANDIDATES = C.  With M > C the candidates at the positions (i M) / C (64-bit integers), i = 0 .. C - 1, are used and
 *     M' = C; otherwise all, M' = M.
 *   Farthest point sampling: selection 0 is candidate 0; every candidate's mind starts at +inf; after each selection s, mind[k] =
 *     min(mind[k], (dx dx + dy dy) + dz dz) with dx = w[k] - w[s], ...; the next selection is the candidate with the largest mind, the
 *     lowest position among equals.  npoints selections; with M' < npoints the rule returns candidate 0 for the rest (every mind is 0).
 * xyz[n][p] is the selected point, index[n][p] its flat pixel slot H W + r W + c (a caller gathers colour or any per-pixel feature with it),
 * count[n] = {M, min(M', npoints)}; with M = 0 the points are zeros and the indices -1.  depth, xyz, index and count follow the handle's I/O
 * mode; cam_ids and bounds are HOST arrays in both modes, passed on by value: the caller may change them as soon as the call returns.  With
 * AVSIM_IO_DEVICE a call synchronises nothing once a call of the same cameras, size and N has run (M stays on the device).  Scratch: the envs
 * go through the kernels in chunks of at most 1024, and a chunk holds min(ncam H W, C) int32 and ncam x 16 floats per env -- at most one
 * int32 per pixel of the chunk, 64 MiB + 1 MiB at the limits, whatever N is.
 * AVSIM_EINVAL, with nothing launched and the outputs untouched: npoints outside 1..4096, height or width outside 1..65535, ncam outside
 * 1..16, ncam H W > 2^24, a bound that is not finite or lo > hi, max_depth not finite or <= 0, a camera id out of range, a null pointer. */
#define AVSIM_PC_MAX_CANDIDATES 16384
int avsim_camera_poses(avsim_t* h, const int32_t* cam_ids, int ncam, float* out /* [N][ncam][16] */);
int avsim_point_cloud(avsim_t* h, const int32_t* cam_ids, int ncam, int height, int width,
                      const float* depth /* [N][ncam][H][W], as avsim_render_depth writes it */,
                      const float bounds[6] /* host: xlo ylo zlo xhi yhi zhi, world */, float max_depth, int npoints,
                      float* xyz /* [N][P][3] */, int32_t* index /* [N][P] */, int32_t* count /* [N][2] */);

/* Voxel grids on the device (csrc/avsim_pointcloud.hip); av_aloha_amd/voxel.py is the specification, and the result equals it
 * bit for bit given the pose records.  One dense grid per env over the box `bounds` in the world frame, from the same depth images, poses
 * (THE CURRENT STATE'S), deprojection and candidate rule as avsim_point_cloud -- d < max_depth, the inclusive box, a NaN drops the pixel --
 * without a cap: every candidate counts.  Per axis, float32, every operation rounded on its own: inv = (float)g / (hi - lo), size =
 * (hi - lo) / (float)g, u = (w - lo) inv, i = min(floor(u), g - 1) (a point on hi goes to the last cell), frac = u - (float)i, q =
 * clip((int)(frac 256), 0, 255).  A cell sums UNSIGNED 32-BIT INTEGERS -- count, q per axis and, with rgb, the pixel's three u8 values --,
 * so the result does not depend on the order of the (atomic) adds and is the same for every call; 2^24 pixels x 255 < 2^32.  Eight float32
 * channels per cell: 0..2 the mean position lo + ((float)i + ((float)sum_q / (float)count + 0.5) (1 / 256)) size, 3..5 the mean colour
 * ((float)sum_c / (float)count) (1 / 255) (0 with rgb NULL), 6 (float)count, 7 occupancy 1.0 / 0.0; an empty cell is eight +0.0.
 * depth, rgb (avsim_render_rgb's env-major u8 layout of the same pixels, or NULL) and out follow the handle's I/O mode; cam_ids, bounds and
 * grid are HOST arrays in both modes, passed on by value.  `out` is the accumulator: no scratch grows with the grid (the pose records of a
 * chunk of at most 1024 envs, shared with avsim_point_cloud, are all there is), and with AVSIM_IO_DEVICE it is 16-byte aligned.
 * AVSIM_EINVAL, with nothing launched and out untouched: ncam outside 1..16, height or width outside 1..65535, ncam H W > 2^24, a grid dim
 * outside 1..AVSIM_VOXEL_MAX_DIM, more than AVSIM_VOXEL_MAX_CELLS cells, a bound that is not finite, lo >= hi on an axis, an extent whose
 * inv or size is not a finite float32, max_depth not finite or <= 0, a camera id out of range, a null cam_ids, depth, bounds, grid or out.
 * The accumulate pass has two forms -- one add per candidate lane, or one per run of consecutive lanes in a cell -- and the build picks one
 * (AVSIM_VOXEL_MERGE, csrc/avsim_pointcloud.hip.h; the merged one unless built otherwise).  Debug option "voxel_other_form" 1 runs the
 * other: the same result, there so that tools/bench_voxel.py can time both in one process. */
#define AVSIM_VOXEL_MAX_DIM 256
#define AVSIM_VOXEL_MAX_CELLS (1 << 21)
int avsim_voxel_grid(avsim_t* h, const int32_t* cam_ids, int ncam, int height, int width,
                     const float* depth /* [N][ncam][H][W] */, const uint8_t* rgb /* [N][ncam][H][W][3], avsim_render_rgb's env-major layout, or NULL */,
                     const float bounds[6] /* host */, float max_depth, const int32_t* grid /* host [3] */, float* out /* [N][gx][gy][gz][8] */);

/* Virtual orthographic views on the device (csrc/avsim_pointcloud.hip); av_aloha_amd/virtviews.py is the specification, and the
 * result equals it bit for bit given the pose records.  What RVT and RVT-2 feed their 2-D transformer: the fused cloud of an env's depth
 * cameras re-rendered into nviews (1..6, repeats allowed) axis-aligned orthographic images of the box `bounds` in the world frame, every one
 * VH x VW (size[0] x size[1], each 1..AVSIM_VV_MAX_SIZE).  Depth images, poses (THE CURRENT STATE'S), deprojection and candidate rule are
 * avsim_point_cloud's -- d < max_depth, the inclusive box, a NaN drops the pixel -- without a cap.  A view is a code 0..5, a proper,
 * unmirrored look at the box from outside (row 0 is the top of the image):
 *   code  name  seen from       column runs along  row runs along   dist
 *   0     +x    the hi-x face   y ascending        z descending     hi_x - w_x
 *   1     -x    the lo-x face   y descending       z descending     w_x - lo_x
 *   2     +y    the hi-y face   x descending       z descending     hi_y - w_y
 *   3     -y    the lo-y face   x ascending        z descending     w_y - lo_y
 *   4     +z    above           x ascending        y descending     hi_z - w_z
 *   5     -z    below           x ascending        y ascending      w_z - lo_z
 * Pixel coordinate, float32 with every operation rounded on its own, for an image axis of n pixels (VW for a column, VH for a row) along
 * world axis k: inv = (float)n / (hi_k - lo_k), u = (w_k - lo_k) inv, i = min(floor(u), n - 1) -- avsim_voxel_grid's cell formula; a point
 * on hi goes to the last pixel --; ascending the pixel is i, descending n - 1 - i.  Footprint: with `radius` r (0..AVSIM_VV_MAX_RADIUS) a
 * candidate at (pr, pc) covers the pixels (pr + dr, pc + dc), |dr|, |dc| <= r, that lie inside the image.  Key: a candidate's key in a view
 * is the UNSIGNED 64-BIT value (bits(dist) << 32) | slot -- the float32 bit pattern of its dist, which is >= 0 inside the box (a point on
 * the face gives +0), above its flat pixel slot H W + r W + c < 2^24.  The winner of a virtual pixel is the SMALLEST key among the
 * candidates that cover it: the nearest point and, among equals, the lowest slot.  A minimum does not depend on the order it is taken in,
 * so the (atomic) scatter gives the same result on every call.
 * out[n][v][r][c] = eight float32: 0..2 the winner's colour (float)u8 * (1.0f / 255.0f) (0 with rgb NULL), 3 its dist in metres, 4..6 its
 * world point -- the deprojection's values for the winning slot, not the pixel's centre --, 7 1.0.  index[n][v][r][c] = the winning slot (a
 * caller gathers any per-pixel feature with it, as with avsim_point_cloud's index).  A pixel nothing covers is eight +0.0 and index -1.
 * depth, rgb (avsim_render_rgb's env-major u8 layout of the same pixels, or NULL), out and index follow the handle's I/O mode; cam_ids,
 * bounds, views and size are HOST arrays in both modes, passed on by value: the caller may change them as soon as the call returns.  `out`
 * is the z-buffer (a pixel's first 8 of its 32 bytes hold the key until the last pass): no scratch beyond the pose records of a chunk of at
 * most 1024 envs, shared with avsim_point_cloud, and with AVSIM_IO_DEVICE nothing synchronises once a call of the same number of cameras
 * has run; there `out` is 16-byte aligned.
 * AVSIM_EINVAL, with nothing launched and both outputs untouched: ncam outside 1..16, height or width outside 1..65535, ncam H W > 2^24,
 * nviews outside 1..6, a view code outside 0..5, a size outside 1..1024, radius outside 0..4, a bound that is not finite, lo >= hi on an
 * axis, an extent whose inv or pixel size (hi_k - lo_k) / (float)n is not a finite float32 -- every axis against both VH and VW, whichever
 * views are named --, max_depth not finite or <= 0, a camera id out of range, out not 16-byte aligned in device mode, a null pointer other
 * than rgb.
 * The scatter pass has two independent cuts, each of which keeps the bits -- a plain load of the pixel's key that skips the atomic when the
 * lane's key is not smaller (keys only decrease: a stale read is safe), and merging runs of consecutive lanes on one virtual pixel in the
 * wave --; all four forms are compiled and the build picks (AVSIM_VV_FORM, csrc/avsim_pointcloud.hip.h: bit 0 the load, bit 1 the merge,
 * 4 the merge always and the load where it was measured to pay: with radius > 0, and with radius 0 when a view has more pixels than the env
 * has source pixels).  4 SHIPS.  Debug option "virtviews_form" f + 1 runs form f (0: the build's) so that tools/bench_virtviews.py can
 * time them in one process. */
#define AVSIM_VV_MAX_VIEWS 6
#define AVSIM_VV_MAX_SIZE 1024
#define AVSIM_VV_MAX_RADIUS 4
int avsim_virtual_views(avsim_t* h, const int32_t* cam_ids, int ncam, int height, int width,
                        const float* depth /* [N][ncam][H][W] */, const uint8_t* rgb /* [N][ncam][H][W][3], avsim_render_rgb's env-major layout, or NULL */,
                        const float bounds[6] /* host */, float max_depth, const int32_t* views /* host [nviews] */, int nviews,
                        const int32_t* size /* host [2]: VH, VW */, int radius, float* out /* [N][nviews][VH][VW][8] */, int32_t* index /* [N][nviews][VH][VW] */);

/* Baseline JPEG streams of rendered frames, encoded on the device (csrc/avsim_jpeg.hip.h): SOF0, 8 bit, JFIF, Y Cb Cr 4:2:0, the Annex K
 * Huffman tables in every frame, one restart interval per MCU row, integer arithmetic throughout -- byte for byte the stream of
 * av_aloha_amd/jpeg.py encode_reference, which is its specification (colour matrix, DCT, quantiser rounding: DESIGN 8.y).
 * avsim_jpeg_bound: worst-case stream length of one height x width image at any quality (header + every coefficient at its longest
 * code, every byte stuffed); AVSIM_EINVAL for a size outside 1..65535.
 * avsim_jpeg_encode: nimg images -> nimg streams.  fmt 0: u8 [nimg][H][W][3] (avsim_render_rgb's layout); fmt 1: float32 [nimg][3][H][W]
 * in [0, 1] (avsim_render_rgb_f32's), turned back into u8 by (int)(v * 255 + 0.5f).  index (may be NULL, int32 [nimg]): encode images
 * index[i] of the batch `img` points to instead of images 0..nimg-1 (a device caller vouches for the range: nothing reads it back).
 * out: u8 [nimg][stride]; out_len: int32 [nimg] = the stream's length.  A stream longer than stride is not written past stride and is
 * invalid; its length still says what it needed.  img, index, out and out_len follow the handle's I/O mode like every other bulk
 * pointer; with AVSIM_IO_DEVICE nothing synchronises once a call of the same size and quality has run.  AVSIM_EINVAL: fmt, quality
 * outside 1..100, height or width < 1 or > 65535. */
int64_t avsim_jpeg_bound(int height, int width);
int avsim_jpeg_encode(avsim_t* h, const void* img, int fmt, const int32_t* index, int nimg, int height, int width, int quality,
                      uint8_t* out, int64_t stride, int32_t* out_len);

/* avsim_render_rgb followed by avsim_jpeg_encode without the pixels leaving the device (a recorder keeps streams, not frames): the visual
 * scene's u8 images of the cameras are rendered into a buffer of the library's and encoded from there.  tile 0: one stream per view of
 * height x width, in avsim_render_rgb's order ([N][ncam], or [ncam][N] under "render_cam_major"); tile 1: the ncam views of an env side
 * by side in ONE height x (ncam * width) image (the Cartesian env's zed_cam = left | right), one stream per env, "render_cam_major" 0.
 * out, stride, out_len as avsim_jpeg_encode.  With host pointers only the lengths and, of every stream, its first min(stride, longest
 * length) bytes come back (the rest of `out` is left as it was); with AVSIM_IO_DEVICE nothing synchronises once a call of the same size
 * has run.  AVSIM_EINVAL: no visual scene, quality outside 1..100, an image size outside 1..65535, tile with "render_cam_major" 1. */
int avsim_render_jpeg(avsim_t* h, const int32_t* cam_ids, int ncam, int height, int width, int tile, int quality, uint8_t* out, int64_t stride,
                      int32_t* out_len);

/* The way back: streams of avsim_jpeg_encode (and of nothing else) -> images on the device, byte for byte the output of
 * av_aloha_amd/jpeg.py decode_reference, its specification.  in: u8 [.][stride], in_len: int32 [.] = each stream's length;
 * stream i of the call is row index[i] of both (index NULL: row i; a device caller vouches for the range).  fmt 0: out = u8
 * [nimg][H][W][3]; fmt 1: float32 [nimg][3][H][W], every value (float)u8 / 255, the bits of avsim_render_rgb_f32.  upsample 0: a chroma
 * sample covers its 2 x 2 pixels (the inverse of the encoder's box filter); 1: libjpeg's h2v2 triangle filter on the chroma plane
 * cropped to ceil(H/2) x ceil(W/2) (what cv2 / Pillow show).  status: int32 [nimg], 0 = a valid image; bit 0: not this encoder's
 * header for (height, width); bit 1: wrong marker structure or length (in_len below header + EOI or above stride, a marker other than
 * RST0..7 in order ceil(H/16) - 1 times, no EOI at the end); bit 2: an entropy error (a code outside the tables, a coefficient index
 * past 63, bytes that run out or are left over, a pad bit that is not 1).  The pixels of a flagged image are unspecified; nothing but
 * its own slot of `out` is written, and no byte string makes the kernels read or write out of bounds.  Pointers follow the handle's
 * I/O mode; with AVSIM_IO_DEVICE nothing synchronises once a call of the same size has run.  AVSIM_EINVAL: fmt, upsample, height or
 * width < 1 or > 65535, stride < 1.  Options: "jpeg_decode_budget" -- bytes of coefficient staging (512 MB); a call that needs more goes
 * through the kernels in groups of images.  "jpeg_decode_events" 1 -- the call records the handle's events 12, 13, 14, 15 before, between
 * and after its three kernels (avsim_event_elapsed_ms(12, 13) = the index kernel, (13, 14) entropy, (14, 15) reconstruction). */
int avsim_jpeg_decode(avsim_t* h, const uint8_t* in, int64_t stride, const int32_t* in_len, const int32_t* index, int nimg, int height, int width,
                      int fmt, int upsample, void* out, int32_t* status);

/* Camera views composed on the device (csrc/avsim_compose.hip.h): images are resampled and written into rectangles of a larger
 * canvas, byte for byte the output of av_aloha_amd/compose.py compose_reference, its specification -- a separable triangle filter whose
 * support grows with the shrink factor (antialiased when shrinking, plain bilinear when enlarging), the horizontal pass first, in Pillow's
 * fixed-point scheme; integer arithmetic on the device, the coefficients computed on the host in double once per size pair.
 * avsim_compose: src = nsrc images of src_h x src_w, fmt 0: u8 [nsrc][H][W][3], fmt 1: float32 [nsrc][3][H][W] in [0, 1], turned into u8 by
 * (int)(v * 255 + 0.5f) as avsim_jpeg_encode does; canvas = nout images of canvas_h x canvas_w, fmt 0: u8 HWC, fmt 1: float32 CHW, every value
 * written (float)u8 / 255, the bits of avsim_render_rgb_f32.  places: int32 [nplace][6] = (out image, src image, x0, y0, w, h): source image
 * `src image` resampled to h x w goes to canvas[out image][y0 : y0 + h][x0 : x0 + w]; the rest of the canvas is left as it is, or, with
 * clear != 0, filled with clear_rgb (0xRRGGBB) first.  One source batch per call: cameras of different sizes are successive calls onto the same
 * canvas with clear set on the first only.  places is a HOST array in both I/O modes (as box / share of avsim_episode_setup) and is checked
 * there; src and canvas follow the handle's I/O mode.  With host pointers and clear = 0 the canvas is copied in before the call and out after
 * it; with AVSIM_IO_DEVICE nothing synchronises once a call with the same sizes and places has run.  AVSIM_EINVAL, with nothing launched
 * and the canvas untouched: a format other than 0 / 1, an image size or a rectangle's w / h outside 1..65535, an image index out of range, a
 * rectangle that does not lie inside the canvas, two rectangles of one output image that overlap (a parallel kernel gives overlaps no
 * order), src_h > 16 h or src_w > 16 w (a shrink of more than 16 per axis; enlarging is unbounded).
 * avsim_compose_label: the text prefix + decimal digits of value[i] painted onto the canvas in the solid colour rgb (0xRRGGBB), label i at
 * where[i] = (out image, x, y, scale): 5 x 7 glyphs in 6 x 8 cells, every glyph pixel a scale x scale square, the first cell's top left
 * corner at (x, y); the canvas is unchanged outside the glyph pixels, and pixels that fall outside the canvas are skipped (a label is clipped,
 * not refused).  Glyphs: 0-9, A-Z, space and : . - = / ; any other character draws as a space.  prefix: a HOST string of at most 15
 * characters (NULL = none); value: int64 [nlabel] following the I/O mode (it may live on the device: the digits are formatted there), NULL =
 * the prefix alone; where: a HOST array.  With host pointers the canvas is copied in and out.  AVSIM_EINVAL: canvas_fmt, canvas size, an
 * image index out of range, scale outside 1..64, |x| or |y| above 2^20, a longer prefix.
 * avsim_compose_font: the glyph table, rows[ch][r] = row r (top first) of character ch, bit 4 = the left pixel, all zero for a character
 * without a glyph; needs no handle and no device (av_aloha_amd/compose.py label_reference draws with this one copy of the font). */
int avsim_compose(avsim_t* h, const void* src, int src_fmt, int nsrc, int src_h, int src_w, void* canvas, int canvas_fmt, int nout, int canvas_h,
                  int canvas_w, const int32_t* places, int nplace, int clear, uint32_t clear_rgb);
int avsim_compose_label(avsim_t* h, void* canvas, int canvas_fmt, int nout, int canvas_h, int canvas_w, const int32_t* where, int nlabel,
                        const char* prefix, const int64_t* value, uint32_t rgb);
void avsim_compose_font(uint8_t rows[128][7]);

/* Training batches on the device (csrc/avsim_imgprep.hip.h); av_aloha_amd/imgprep.py is the specification, and both calls
 * equal it bit for bit.  Images are fmt 0: u8 [n][H][W][3] or fmt 1: float32 [n][3][H][W] in [0, 1], read as u8 by (int)(v * 255 + 0.5f)
 * as avsim_jpeg_encode does.
 * avsim_image_stats: out[i][c] = (sum, sum of squares, min, max) of the u8 values of channel c of image index[i] (index NULL: image i), as
 * uint64 -- the integers a data set's mean / std / min / max are made of (imgprep.combine_stats), exact and the same on every run.  img,
 * index and out follow the handle's I/O mode; a host caller's index is checked (negative: AVSIM_EINVAL) and says how many images img
 * holds, a device caller's is not read by the host.  AVSIM_EINVAL, with nothing launched and out untouched: fmt other than 0 / 1, height or
 * width outside 1..65535, nimg < 1.
 * avsim_image_prep: out[i][c][y][x] = lut[lut_index[i]][c][u8(img[src_index[i]])[y0 + y][x0 + (flip ? out_w - 1 - x : x)][c]] with
 * (x0, y0, flip) = box[i]: a crop, an optional mirror and a per-channel table look-up in one pass -- normalisation ((u / 255 - mean) / std
 * tabulated, imgprep.normalise_lut), brightness, gamma, any per-channel curve.  lut: float32 [nlut][3][256]; lut_index NULL: table 0 for every
 * output; src_index NULL: output i reads image i.  img, lut and out follow the handle's I/O mode; box, lut_index and src_index are HOST arrays
 * in both modes (as avsim_compose's places), checked before anything is launched and copied into pinned staging of the library's own before
 * the call returns -- the caller may change or free them at once.  The staging is reused behind events: with AVSIM_IO_DEVICE a call does not
 * synchronise the stream once a call of the same sizes has run.  AVSIM_EINVAL, with nothing launched and out untouched: fmt other than 0 / 1,
 * an image or output size outside 1..65535, a crop that does not lie inside the source, a flip other than 0 / 1, a lut_index outside
 * [0, nlut), a src_index outside [0, nsrc), nsrc, nout or nlut < 1 (nlut at most 2^20). */
int avsim_image_stats(avsim_t* h, const void* img, int fmt, const int32_t* index, int nimg, int height, int width, uint64_t* out /* [nimg][3][4] */);
int avsim_image_prep(avsim_t* h, const void* img, int fmt, int nsrc, int height, int width, const float* lut, int nlut, const int32_t* lut_index,
                     const int32_t* box /* [nout][3] */, int nout, const int32_t* src_index, int out_h, int out_w,
                     float* out /* [nout][3][out_h][out_w] */);

/* Colour and sharpness augmentation of training images on the device (csrc/avsim_imgaug.hip); av_aloha_amd/imgaug.py is the
 * specification, and the call equals it bit for bit (-0 and +0 aside).
 * avsim_image_jitter: output i is image src_index[i] (NULL: image i) of img with the operations of mask = box_mask[i][3] applied to the WHOLE
 * image -- bit 0 brightness, 1 contrast, 2 saturation, 3 hue, 4 sharpness, in that order, with the factors factor[i] = (fb, fc, fs, fh, fsh),
 * torchvision's adjust_* arithmetic for float images in float32, floats carried from one operation to the next --, then cropped and
 * mirrored by (x0, y0, flip) = box_mask[i][0..2] as avsim_image_prep crops, then normalised per channel as (v - mean[c]) / std[c] with
 * mean_std = (mean[3], std[3]); mean_std NULL: the values stay in [0, 1].  Contrast blends with the mean gray of the whole source image
 * (after brightness), reduced in integers first; sharpness blends with a 3 x 3 blur whose border is the source image's, not the crop's.
 * Only u8 [nsrc][H][W][3] images are read (the float CHW format stays with avsim_image_prep).  img and out follow the handle's I/O mode;
 * box_mask, factor, src_index and mean_std are HOST arrays in both modes, checked before anything is launched and copied into the pinned
 * staging avsim_image_prep uses before the call returns -- the caller may change or free them at once.  With AVSIM_IO_DEVICE a call does
 * not synchronise the stream once a call of the same sizes has run.  AVSIM_EINVAL, with nothing launched and out untouched: an image or
 * output size outside 1..65535, nsrc or nout < 1, a crop that does not lie inside the source, a flip other than 0 / 1, a mask outside 0..31, a
 * src_index outside [0, nsrc), a factor of a set bit that is not finite, a brightness, contrast, saturation or sharpness factor of a set bit
 * outside [0, 16], a hue factor of a set bit outside [-0.5, 0.5], a std that is 0 or not finite.  Factors of unset bits are not looked at.
 * avsim_image_jitter_sums (for tests): sums[i] = the integer S behind output i's contrast mean in the last avsim_image_jitter call of this
 * handle, m = float(double(S) / double(H W 2^20)), for the outputs that had the contrast bit (the other slots hold nothing meant); sums: a HOST
 * array of nout <= that call's nout values in both modes.  Synchronises the stream. */
int avsim_image_jitter(avsim_t* h, const void* img /* u8 [nsrc][H][W][3] */, int nsrc, int height, int width,
                       const int32_t* box_mask /* [nout][4]: x0, y0, flip, mask */, const float* factor /* [nout][5] */,
                       const int32_t* src_index /* or NULL */, int nout, const float* mean_std /* [2][3] or NULL: [0,1] output */,
                       int out_h, int out_w, float* out /* [nout][3][out_h][out_w] */);
int avsim_image_jitter_sums(avsim_t* h, uint64_t* sums /* [nout] */, int nout);

/* avsim_image_jitter with the geometric op of LeRobot's image_transforms, torchvision's RandomAffine with fill 0 (csrc/avsim_imgaug.hip; DESIGN
 * 8.af); av_aloha_amd/imgaug.py (jitter_affine_reference) is the specification, and the call equals it bit for bit (-0 and +0 aside).
 * avsim_image_augment: everything as avsim_image_jitter, and mask bit 5 (32): after the colour operations and sharpness, still on the WHOLE
 * image and before the crop, output i is resampled through the float32 inverse matrix M = affine[i]: with xf = (x + 0.5) - W / 2 and
 * yf = (y + 0.5) - H / 2, the pixel (x, y) reads the source position sx = M0 xf + M1 yf + M2 + (W / 2 - 0.5), sy = M3 xf + M4 yf + M5 +
 * (H / 2 - 0.5) (imgaug.py names every rounding; imgaug.affine_matrix makes M from an angle, a translation, a scale and shears).  interp, one
 * per call: 0 the nearest pixel (half to even), 1 bilinear.  A tap outside the image is 0 in every channel, and is normalised like any other
 * value.  affine is a HOST array like factor and may be NULL when no mask has bit 5; the entries of an output without the bit are not read.
 * Without bit 5 anywhere the call runs avsim_image_jitter's kernels.  Outputs that have sharpness and bit 5 go through float images of the
 * library's, at most 128 MiB of them at a time (option "augment_scratch_bytes"; one whole image at least), grown on demand.  AVSIM_EINVAL,
 * with nothing launched and out untouched: avsim_image_jitter's conditions with masks 0..63, an interp other than 0 / 1, a matrix entry of a
 * set bit 5 that is not finite or larger than 2^20 in magnitude, affine NULL with a bit 5 set.  avsim_image_jitter_sums reads this call's sums too. */
int avsim_image_augment(avsim_t* h, const void* img /* u8 [nsrc][H][W][3] */, int nsrc, int height, int width,
                        const int32_t* box_mask /* [nout][4]: x0, y0, flip, mask */, const float* factor /* [nout][5] */,
                        const float* affine /* [nout][6] or NULL */, int interp, const int32_t* src_index /* or NULL */, int nout,
                        const float* mean_std /* [2][3] or NULL: [0,1] output */, int out_h, int out_w, float* out /* [nout][3][out_h][out_w] */);

/* Resizing images on the device, antialiased, into a rectangle of a padded output (csrc/avsim_imgresize.hip);
 * av_aloha_amd/imgresize.py (resize_reference) is the specification, and the call equals it bit for bit (-0 and +0 aside).
 * avsim_image_resize: output i reads image src_index[i] (NULL: image i) of img -- fmt 0: u8 [nsrc][H][W][3] with value float(u) / 255, fmt 1:
 * float32 [nsrc][3][H][W] read AS FLOATS (not quantised as avsim_image_prep quantises, so that an avsim_image_jitter output resizes without a
 * loss).  src_box[i] = (x0, y0, w, h, flip) is the source region and dst[i] = (ox, oy, rw, rh) the rectangle of the out_h x out_w output
 * that the resized region fills; every other output pixel is fill[c] (fill NULL: 0).  The filter is the separable triangle filter of torch's
 * interpolate(mode="bilinear", align_corners=False, antialias=...): per axis and output index i, in float32, scale = n_in / n_out, support =
 * scale when antialias and scale >= 1, else 1, center = scale (i + 0.5), the taps j from max(0, int(center - support + 0.5)) to min(n_in,
 * int(center + support + 0.5)) with weights max(0, 1 - |(j - center + 0.5) inv|), inv = 1 / support, over their sum; n_in is the REGION's size, so no
 * pixel outside the box is read and crop-then-resize equals resizing the crop.  The horizontal pass comes first, then the vertical one, each a
 * sum of products in ascending j with no fused multiply-add.  flip mirrors the resized rectangle; last every output pixel, fill included,
 * becomes (v - mean[c]) / std[c] with mean_std = (mean[3], std[3]) (NULL: the values stay).  Upscaling is allowed; a ratio w / rw or h / rh
 * above 16 is refused.  img and out follow the handle's I/O mode; src_box, dst, src_index, fill and mean_std are HOST arrays in both modes,
 * checked before anything is launched and copied (52 bytes per output and 48 per call) into the pinned staging avsim_image_prep uses before
 * the call returns -- the caller may change or free them at once.  With AVSIM_IO_DEVICE a call does not synchronise the stream once a call
 * of the same sizes has run.  AVSIM_EINVAL, with nothing launched and out untouched: a fmt other than 0 / 1, an image or output size outside
 * 1..65535, nsrc or nout < 1, a source box that does not lie inside the image, a dst rectangle that does not lie inside the output, w, h, rw or
 * rh < 1, a ratio above 16, a flip or an antialias other than 0 / 1, a src_index outside [0, nsrc), a fill that is not finite, a std that is 0
 * or not finite. */
int avsim_image_resize(avsim_t* h, const void* img, int fmt, int nsrc, int height, int width,
                       const int32_t* src_box /* [nout][5]: x0, y0, w, h, flip */, const int32_t* dst /* [nout][4]: ox, oy, rw, rh */,
                       const int32_t* src_index /* or NULL */, int nout, int antialias, const float* fill /* [3] or NULL: 0 */,
                       const float* mean_std /* [2][3] or NULL */, int out_h, int out_w, float* out /* [nout][3][out_h][out_w] */);

/* Per-env episodes on the device (a vector env with gymnasium's NEXT_STEP autoreset; av_aloha_amd/vec_env.py).  Pointers follow the
 * handle's I/O mode, except box / share of the set-up (host pointers).  In device mode no step, reset, sample or render call
 * synchronises; avsim_episode_setup does (it reallocates the records: once per evaluation), and so do avsim_episode_log /
 * avsim_episode_count given host pointers.
 *
 * avsim_episode_setup: box = double[nobj][6] (lo xyz, hi xyz of every free object's initial position, qpos order), share = int32[nobj]
 * (-1, or the index of an earlier object whose position this one takes: TubeTransfer's tube1 and ball), seed; an episode ends after
 * max_episode_steps steps (truncated) or, with terminate_on_success, at success (terminated); the records of episode ids
 * [0, log_capacity) are kept.  Clears the id counter and the records; every env starts an episode at its next reset / step.
 * Initial poses: Philox4x32-10 with key = seed and counter = (episode id, object index, 0); coordinate k of an object's block x gives
 * u = (x_k + 0.5) 2^-32 and pos = lo + (hi - lo) u in double (each operation rounded); identity orientation.  They depend on
 * (seed, episode id) only. */
int avsim_episode_setup(avsim_t* h, const double* box, const int32_t* share, uint64_t seed, int max_episode_steps,
                        int terminate_on_success, int64_t log_capacity);
/* the sampler as a pure function: obj_qpos double[n][nobj][7] of episode_id int64[n] under `seed` (the set-up's boxes) */
int avsim_sample_poses(avsim_t* h, uint64_t seed, int n, const int64_t* episode_id, double* obj_qpos);
/* envs with mask[i] != 0 (uint8[N]; NULL = all) start an episode now: the next ids of the counter in env-index order, the state of
 * avsim_reset at that episode's poses (no forward pass: a step starts from qpos, qvel, ctrl, warmstart and latch alone).  agent_pos
 * double[N][nj] and episode_id int64[N] of every env (either may be NULL). */
int avsim_episode_reset(avsim_t* h, const uint8_t* mask, double* agent_pos, int64_t* episode_id);
/* avsim_step, then the episode bookkeeping.  An env whose episode ended in the previous call (NEXT_STEP) starts its next episode in
 * this one: the action does not reach it, and it reports reward 0, success / terminated / truncated 0, elapsed 0, its new id and the
 * new state's agent_pos (avsim_observe after avsim_reset of the same poses, bit for bit).  The others report the step with elapsed =
 * steps of the episode so far; truncated = elapsed reached max_episode_steps or the state diverged (avsim_get_diag bit 0).  Outputs:
 * agent_pos double[N][nj], reward int32[N], success / terminated / truncated uint8[N], episode_id int64[N], elapsed int32[N]; any may
 * be NULL. */
int avsim_episode_step(avsim_t* h, const float* action, int nsub, double* agent_pos, int32_t* reward, uint8_t* success,
                       uint8_t* terminated, uint8_t* truncated, int64_t* episode_id, int32_t* elapsed);
/* records of episode ids [0, n), n <= log_capacity: return double, length int32 (0 = not finished yet), max reward int32, success seen
 * uint8, initial object poses double[nobj][7]; any may be NULL */
int avsim_episode_log(avsim_t* h, int64_t n, double* ret, int32_t* length, int32_t* max_reward, uint8_t* success, double* obj_qpos0);
/* count = {episodes started, episodes finished} since avsim_episode_setup */
int avsim_episode_count(avsim_t* h, int64_t count[2]);

/* Per-env execution of a policy's action chunks on the device (csrc/avsim_chunks.hip); av_aloha_amd/chunks.py is the
 * specification, and the calls equal it bit for bit.  One state per handle, sized to its num_envs.  A policy predicts chunks
 * float [N][C][A] of normalised actions, row k of env i its action k steps from now; avsim_chunk_step turns them into the float [N][A]
 * action of avsim_episode_step.  Env i is FRESH in a call when it has not been stepped since the set-up / avsim_chunk_reset, or
 * elapsed[i] == 0, or episode_id[i] differs from the id the previous call saw: its state starts empty.  Every value is un-normalised first,
 * y = x * std[a] + mean[a] (two float32 operations; mean_std NULL: y = x).
 * mode 0, ensemble (LeRobot's ACTTemporalEnsembler, online): with u = the env's updates since fresh, for k in 0 .. C-1, c = min(u, C-1-k),
 * slot j = (u + k) mod C: ens[j] = y[k] if c == 0, else (ens[j] * cum[c-1] + y[k] * w[c]) / cum[c], every operation a float32 one rounded
 * on its own; the action is ens[u mod C].  tables = (w[C], cum[C]) are the caller's (chunks.ensemble_tables): the library computes no exp.
 * mode 1, queue: an env NEEDS a chunk when it is fresh or its queue is empty; it then takes rows [first, first + n_action_steps) of its
 * chunk and returns them one per call.  With chunks NULL such an env is STARVED: it repeats its previous action (zeros if fresh), its queue
 * stays empty and the counter of avsim_chunk_starved goes up by one.  An env that does not need a chunk ignores the one given.
 * avsim_chunk_setup: tables and mean_std are HOST arrays, copied before the call returns; everything is checked before anything is
 * allocated or enqueued -- AVSIM_EINVAL: chunk_size outside 1..1024, action_dim outside 1..64, mode other than 0 / 1, queue: n_action_steps
 * < 1, first < 0, first + n_action_steps > chunk_size; ensemble: tables NULL, an entry not finite, a cum[c] <= 0; a mean or std not finite.
 * (Re)initialises the state: all envs unstepped, the starved counter 0.  Synchronises.  avsim_chunk_reset: all envs unstepped.
 * avsim_chunk_need: need uint8 [N] and any int32 [1] (1 when some env needs; either may be NULL) from one kernel; changes no state; in
 * ensemble mode every env needs a chunk in every call.  avsim_chunk_step: chunks NULL in ensemble mode, or any of these calls before the
 * set-up, is AVSIM_EINVAL with nothing enqueued and the state untouched.  The array pointers of need / step follow the handle's I/O mode;
 * the work goes on the handle's stream, and with AVSIM_IO_DEVICE neither synchronises.  avsim_chunk_starved: count is a HOST pointer;
 * synchronises, like avsim_episode_count. */
int avsim_chunk_setup(avsim_t* h, int chunk_size, int action_dim, int mode, int n_action_steps, int first,
                      const float* tables /* host [2][C] or NULL */, const float* mean_std /* host [2][A] or NULL */);
int avsim_chunk_reset(avsim_t* h);
int avsim_chunk_need(avsim_t* h, const int64_t* episode_id, const int32_t* elapsed, uint8_t* need /* [N] */, int32_t* any /* [1] */);
int avsim_chunk_step(avsim_t* h, const float* chunks /* [N][C][A] or NULL */, const int64_t* episode_id /* [N] */,
                     const int32_t* elapsed /* [N] */, float* action /* [N][A] */);
int avsim_chunk_starved(avsim_t* h, uint64_t* count);

/* Per-env observation histories on the device (csrc/avsim_obshist.hip); av_aloha_amd/obshist.py is the specification, and the
 * calls equal it bit for bit.  One state per handle, sized to its num_envs.  A policy with n_obs_steps = K reads [N][K][...]: slot K-1 is
 * the newest observation.  Env i is FRESH in a call exactly as for avsim_chunk_step: not pushed since the set-up / avsim_obs_history_reset,
 * or elapsed[i] == 0, or episode_id[i] differs from the id the previous call saw.  Per call and env, the new state is (x - mean[d]) / std[d]
 * (two float32 operations; state_mean_std NULL: x) and the new image of camera c is avsim_image_prep's with table lut[c] and box[c] =
 * (x0, y0, flip), from img[c] in format fmt (0: uint8 [N][height][width][3], 1: float32 [N][3][height][width]).  A fresh env: all K slots
 * become the new value and the old contents are not read; otherwise slot[k] = slot[k+1] for k < K-1 and slot[K-1] = new.
 * avsim_obs_history_setup: state_mean_std, lut and box are HOST arrays, copied before the call returns; everything is checked before
 * anything is allocated or enqueued -- AVSIM_EINVAL: n_obs_steps outside 1..16, state_dim outside 0..256, ncam outside 0..8, state_dim 0
 * with ncam 0, and with cameras: fmt other than 0 / 1, a size outside 1..65535, lut or box NULL, a crop not inside the source, a flip
 * other than 0 / 1; a mean not finite, a std 0 or not finite.  (Re)initialises the state: all envs unpushed.  Synchronises.
 * avsim_obs_history_push: img and img_hist are HOST arrays of ncam pointers; the arrays they name, and state float [N][D], state_hist float
 * [N][K][D], img_hist[c] float [N][K][3][out_h][out_w], episode_id and elapsed, follow the handle's I/O mode.  The histories are the
 * caller's memory, updated in place.  AVSIM_EINVAL, with nothing enqueued and the state untouched: a push or reset before the set-up, a NULL
 * id array, a NULL state or state_hist with state_dim > 0, a NULL camera pointer.  The work goes on the handle's stream; with
 * AVSIM_IO_DEVICE neither push nor reset synchronises.  Without it every array, the histories included, is copied to the device and the
 * histories back around the pass: that mode is for tests and numpy callers.  16-byte history accesses when out_h out_w is a multiple of
 * four and every img_hist[c] is 16-byte aligned, single floats otherwise. */
int avsim_obs_history_setup(avsim_t* h, int n_obs_steps, int state_dim, const float* state_mean_std /* host [2][D] or NULL */, int ncam, int fmt,
                            int height, int width, const float* lut /* host [ncam][3][256] */, const int32_t* box /* host [ncam][3] */,
                            int out_h, int out_w);
int avsim_obs_history_reset(avsim_t* h);
int avsim_obs_history_push(avsim_t* h, const int64_t* episode_id /* [N] */, const int32_t* elapsed /* [N] */, const float* state,
                           float* state_hist, const void* const* img /* host [ncam] */, float* const* img_hist /* host [ncam] */);

/* get_reward of the handle's task (gym_guided_vision/gym_guided_vision/env.py:425-863, five subclasses) evaluated on
 * caller-supplied contact lists instead of the simulator's own contacts: geom_pairs = int32[nsets][cap][2], ids into the
 * model's collision geom table (manifest "geom_names"), a slot with a negative id is empty.  The kernel applies the same
 * predicate as the step kernel.  latch (may be NULL = all zero) is int32[nsets], read and updated in place (SewNeedle's
 * threaded_needle, env.py:596); reward = int32[nsets].  All pointers are host pointers. */
int avsim_reward_from_pairs(avsim_t* h, const int32_t* geom_pairs, int nsets, int cap, int32_t* latch, int32_t* reward);

/* stream / timing helpers (HIP events on the stream the kernels are launched on) */
int avsim_sync(avsim_t* h);
int avsim_set_stream(avsim_t* h, void* hip_stream);
int avsim_event_record(avsim_t* h, int slot);                            /* slot in [0,16) */
int avsim_event_elapsed_ms(avsim_t* h, int slot_a, int slot_b, float* ms); /* synchronises on slot_b */
/* accumulated device time of the physics kernel since the last call with reset!=0, measured with
 * HIP events around every launch (on the launch stream, no per-launch synchronisation) when enabled via
 * avsim_set_option("kernel_timing", 1); this call synchronises on the recorded events */
int avsim_kernel_time(avsim_t* h, int reset, double* total_ms, int64_t* launches);
/* the same for the image kernel of avsim_render_depth / avsim_render_labels / the proxy mode of avsim_render_rgb (k_render_depth alone: the pose pass
 * and the per-view set-up kernel in front of it are not in the figure) */
int avsim_render_kernel_time(avsim_t* h, int reset, double* total_ms, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif
