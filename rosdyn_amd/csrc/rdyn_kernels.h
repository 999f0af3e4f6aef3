// rdyn_kernels.h -- launch interface between the C-ABI layer (rdyn_api*.cpp) and the HIP kernels.
#ifndef RDYN_KERNELS_H
#define RDYN_KERNELS_H

#include <hip/hip_runtime.h>
#include "rdyn_device.h"

// All strides are in doubles.  Inputs: x(s, k) = x[s * in_ss + k * in_sj].
struct RdynSweepArgs
{
  const RdynChainConst* chain;  // device pointer
  const double *q, *dq, *ddq;   // dq / ddq may be null (treated as zero)
  int64_t n_samples;
  int64_t in_ss, in_sj;
  double* tau;                  // may be null in regressor mode
  int64_t tau_ss, tau_sj;
  double* Y;
  int64_t y_ss, y_sr, y_sc;
  double* M;
  int64_t m_ss, m_se;
  // regressor mode only: optional measured torque, copied into regressor column P (the "b" column of the
  // normal equations) with the Y addressing; same layout as q.
  const double* bcol;
  int bcol_col;                 // column that receives bcol; 0 = column P (right after the regressor)
  // torque mode only: optional external wrenches, links x 6 per sample ([force; torque] in the link's own frame,
  // applied TO the link; getWrench, primitives_impl.h:1225); element e of sample s at ext[s * ext_ss + e * ext_se]
  const double* ext;
  int64_t ext_ss, ext_se;
  // RDYN_MODE_REGRESSOR_EXPAND only (a chain longer than what the kernels sweep: `chain` is its reduced companion): the ten columns of
  // chain link g are the columns of reduced link expand_red_of[g] times the constant 10 x 10 block X_g (rdyn_chain.hpp), zero for links
  // upstream of the first input joint (expand_red_of[g] < 0).  expand_X: device, [expand_n][10][10] row-major X_g(a, p).
  const double* expand_X;
  int expand_n;
  int expand_red_of[RDYN_MAX_JOINTS];  // (ints: a dynamically indexed byte of the kernel arguments is a VECTOR load, whose wait drains every store in flight)
  // RDYN_MODE_REGRESSOR_EXPAND_STAGED: the row-contiguous layout the wave's LDS tile is copied out to -- 1: per-sample images
  // (stride_col == rows, a link's block is one run of 10 rows doubles per sample), 2: stacked matrix (stride_sample == rows, a column is
  // one run of 64 rows doubles per wave)
  int expand_stage;
  // per-sample images through a run-time row map (k_image_sweep<.., MAP>: input joints in any order -- `chain` is then the sorted view,
  // rdyn_chain.hpp -- and joints that are not input joints anywhere in the chain): row_map[f] = the caller's input index of chain joint
  // f -- where q / Dq / DDq are read, tau is written, and the row of the image its values land in --, -1 for a joint that is none
  int row_map[RDYN_MAX_SWEPT_JOINTS];
  // k_image_sweep<.., EXPAND>: the links of the full chain that ride on body f are expand_first[f] .. expand_first[f + 1] - 1 (chain order;
  // the links below expand_first[0] sit upstream of the first input joint: zero blocks)
  int expand_first[RDYN_MAX_SWEPT_JOINTS + 1];
  // torque / inertia launches: the sample-major records (tau: n, M: n x n doubles per sample) through the wave's LDS tile, written in whole
  // lines (rdyn_record_stage.h); decided by the host: natural strides, 128-byte aligned output
  int staged;
  // k_image_sweep: chunk permutation of the workgroups (0 = none), see rdyn_image_impl.h
  unsigned blk_mul;
};

// split / jerk sweeps (rdyn_kin_ext.hip); every output record is links x 6
struct RdynKinExtArgs
{
  const RdynChainConst* chain;
  const double *q, *dq, *ddq, *dddq;
  int64_t n_samples, in_ss, in_sj;
  int64_t out_ss, out_se;
  double* dtw_lin;
  double* dtw_nonlin;
  double* ddtw;
  double* ddtw_lin;     // getDDTwistLinearPart
  double* ddtw_nonlin;  // getDDTwistNonLinearPart
  double* wrench;       // getWrench: base-frame link wrenches
  const double* ext;    // wrench only, may be null: external wrenches, links x 6, element e of sample s at ext[s * ext_ss + e * ext_se]
  int64_t ext_ss, ext_se;
  // rdyn_long_kin.hip only (chains of more than RDYN_MAX_SWEPT_JOINTS joints): the constants and the joint torques of the wrench pass
  // (getJointTorque with external wrenches; layout of q)
  const RdynLongChainConst* chain_long;
  double* tau;
  int64_t tau_ss, tau_sj;
  int staged;  // sample-major records through wave-private LDS, whole lines (rdyn_record_stage.h); decided by the host: natural strides, line-aligned outputs
  int ext_staged;  // ... and the external wrenches read as whole lines into the same tile (16-byte aligned, natural stride)
  int ext_one;     // rdyn_long_kin.hip only: 0 = ext holds links x 6 per sample; 1 + l = 6 per sample, applied to chain link l alone
};
hipError_t rdyn_launch_base_ext(int n_joints, const RdynKinExtArgs& a, hipStream_t st);
hipError_t rdyn_launch_long_ext(int n_joints, const RdynKinExtArgs& a, hipStream_t st);  // a.chain_long; any chain length

// batched local inverse kinematics (rdyn_ik.hip)
struct RdynIkArgs
{
  const RdynChainConst* chain;
  const double* T_target;            // 12 per pose, column-major 3x4 [R | p]; element e of pose s at [s * tt_ss + e * tt_se]
  int64_t tt_ss, tt_se;
  const double* seed;                // n_active per pose, x(s, k) = seed[s * in_ss + k * in_sj]
  double* sol;                       // same addressing as seed (may alias it)
  int64_t n_samples, in_ss, in_sj;
  double weight[6];                  // all 1 for computeLocalIk
  double q_min[RDYN_MAX_SWEPT_JOINTS];     // per CHAIN joint
  double q_max[RDYN_MAX_SWEPT_JOINTS];
  // a constant frame behind the last swept joint (a chain served through its reduced companion: the fixed frames after the last
  // input joint): T_tool = T_last [tail_R | tail_t]; tail_R row-major
  int has_tail;
  double tail_R[9], tail_t[3];
  double toll;
  double damping;                    // Levenberg term: damping^2 is added to the diagonal of J'WJ (0 = the reference's QP)
  int max_iter;
  int it_stage;                      // > 0: resume launch -- continue the poses a first launch left unfinished after it_stage updates
  int* status;                       // per pose, may be null: 1 converged, 0 not within max_iter, < 0 QP failure
  int* iterations;                   // per pose, may be null: QP updates performed
};
hipError_t rdyn_launch_local_ik(int n_joints, const RdynIkArgs& a, hipStream_t st);

// the same loop for a chain of more than RDYN_MAX_SWEPT_JOINTS joints with more input joints than its reduced companion holds
// (rdyn_long_ik.hip: rolled link loop, the Jacobian columns in wave-private LDS, the QP through a 6 x 6 system).  The QP variables are
// the moving input joints in CHAIN order.
struct RdynLongIkArgs
{
  const RdynLongChainConst* chain_long;
  const double* T_target;            // as in RdynIkArgs
  int64_t tt_ss, tt_se;
  const double* seed;
  double* sol;                       // may alias seed
  int64_t n_samples, in_ss, in_sj;
  double weight[6];
  int n_var;                         // QP variables (<= RDYN_MAX_JOINTS)
  int var_in[RDYN_MAX_JOINTS];       // per variable: its index in the input vectors
  double q_min[RDYN_MAX_JOINTS];     // per variable
  double q_max[RDYN_MAX_JOINTS];
  double toll;
  double damping;
  int max_iter;
  int* status;                       // may be null
  int* iterations;                   // may be null
};
size_t rdyn_long_ik_lds_bytes(int n_var);  // dynamic LDS of one 64-lane workgroup
hipError_t rdyn_launch_long_ik(const RdynLongIkArgs& a, hipStream_t st);

// getFrameDistance family (frame_distance.h) on pairs of frames; element e of record s at base[s * X_ss + e * X_se]
struct RdynFrameDistanceArgs
{
  const double *T_wa, *T_wb;   // 12 per frame, column-major 3x4 [R | p]
  int64_t n, t_ss, t_se;
  int kind;                    // 0 getFrameDistance, 1 getFrameDistanceQuat, 2 getFrameDistanceQuatJac
  double* distance;            // 6 per pair
  int64_t d_ss, d_se;
  double* jacobian;            // kind 2 only, may be null: 36 per pair, column-major 6 x 6
  int64_t j_ss, j_se;
};
hipError_t rdyn_launch_frame_distance(const RdynFrameDistanceArgs& a, hipStream_t st);

// Base-frame kinematics outputs; record element e of sample s at out[s * X_ss + e * out_se].
struct RdynKinArgs
{
  const RdynChainConst* chain;
  const double *q, *dq, *ddq;
  int64_t n_samples;
  int64_t in_ss, in_sj;
  int64_t out_se;
  double* T_bt;    int64_t tb_ss;   // 12 per sample
  double* T_links; int64_t tl_ss;   // 12 * links per sample
  double* J;       int64_t j_ss;    // 6 * n_active per sample
  int j_link;                       // Jacobian reference link (chain link index); n_joints = the tool (getJacobian)
  double* twists;                   // 6 * links per sample
  double* dtwists; int64_t tw_ss;
  // rdyn_long_kin.hip only (chains of more than RDYN_MAX_SWEPT_JOINTS joints): the constants; j_up = input joints upstream of link
  // j_link (the first j_up input columns of the Jacobian are filled, primitives_impl.h:965-972)
  const RdynLongChainConst* chain_long;
  int j_up;
  // sample-major records through wave-private LDS, written in whole lines (rdyn_record_stage.h): natural record strides (out_se == 1,
  // X_ss = the record length) and every output pointer 128-byte aligned -- decided by the host; n_active sizes the Jacobian's tile
  int staged;
  int n_active;
};
hipError_t rdyn_launch_long_base(const RdynKinArgs& a, hipStream_t st);

// regressor (+ fused torque) / joint inertia of a chain with more input joints than the unrolled kernels sweep (rdyn_long_local.hip)
struct RdynLongLocalArgs
{
  const RdynLongChainConst* chain_long;
  const double *q, *dq, *ddq;   // dq / ddq may be null (zero)
  int64_t n_samples, in_ss, in_sj;
  double* tau;                  // regressor mode, may be null
  int64_t tau_ss, tau_sj;
  double* Y;
  int64_t y_ss, y_sr, y_sc;
  double* M;
  int64_t m_ss, m_se;
  // regressor mode, may be null: the measured torque (layout of q), copied into regressor column bcol_col with the Y addressing -- the
  // "b" column of the chunk images rdyn_regressor_gram hands to k_gram
  const double* bcol;
  int bcol_col;
  // regressor mode: 1 = per-sample images (stride_row 1, stride_col n_active), 2 = the stacked matrix (stride_sample n_active) -- a link's
  // block through a wave-private LDS tile two columns at a time, copied out 16 bytes per lane; 0 = stores from the computing lane
  int stage;
  int n_active;
};
size_t rdyn_long_local_lds_bytes(int mode, int n_joints);
hipError_t rdyn_launch_long_local(int mode, int n_joints, const RdynLongLocalArgs& a, hipStream_t st);  // mode: RDYN_MODE_REGRESSOR / RDYN_MODE_INERTIA

// forward dynamics (rdyn_fwd_dyn.hip): ddq = M^-1 (tau - h); tau, ddq addressed like q (ddq may alias tau)
struct RdynFwdDynArgs
{
  const RdynChainConst* chain;
  const double *q, *dq, *tau;
  double* ddq;
  int32_t* status;  // may be null: 1 solved, -1 M not positive definite (the sample's ddq is NaN)
  int64_t n_samples, in_ss, in_sj;
  int staged;       // doubles per record (n_active): sample-major records through the wave's LDS tile (natural strides, line-aligned ddq); 0 = 8-byte stores
};
hipError_t rdyn_launch_forward_dynamics(int n_joints, const RdynFwdDynArgs& a, hipStream_t st);
// ... of a chain with more input joints than the unrolled kernels sweep: in-place Cholesky of one element-major chunk image [M | h]
// (element (i, j) of sample s of the chunk at image[(i n + j) ld + s], h_i at image[(n n + i) ld + s]) and the two triangular solves
struct RdynFwdSolveArgs
{
  double* image;
  int64_t ld;
  int n;
  const double* tau;  // the chunk's first sample
  double* ddq;
  int32_t* status;    // may be null
  int64_t n_samples, in_ss, in_sj;  // samples of the chunk (<= ld)
};
hipError_t rdyn_launch_forward_solve(const RdynFwdSolveArgs& a, hipStream_t st);

// rollouts (rdyn_rollout.hip): T integrator steps of the forward dynamics from (q, dq) under the torques tau + t * tau_step (addressed like q)
struct RdynRolloutArgs
{
  const RdynChainConst* chain;
  const double *q, *dq, *tau;
  int64_t tau_step;           // doubles between the torques of consecutive steps (0: the same at every step)
  double *q_end, *dq_end;     // may be null; may alias q / dq
  double *q_traj, *dq_traj;   // may be null: record k = the state after step (k + 1) traj_every at + k * traj_step
  int64_t traj_step;
  int32_t* status;            // may be null: 1, or -1 from the first evaluation on that failed the pivot rule (the state is NaN from that step on)
  int64_t n_samples, in_ss, in_sj;
  double dt;
  int n_steps, traj_every, integrator, n_active;
  int staged;  // sample-major records through the wave's LDS tile in whole lines (natural strides, line-aligned): bit 0 the end state, bit 1 the trajectory
};
hipError_t rdyn_launch_rollout(int n_joints, const RdynRolloutArgs& a, hipStream_t st);
// ... of a chain with more input joints than the unrolled kernels sweep: the element-wise update after one forward-dynamics pass (stage
// `stage` of the step; Euler has one).  Every array holds count = n * n_samples doubles in the batch's layout.
struct RdynRolloutStageArgs
{
  double *q, *dq;             // the step's state: advanced at the last stage
  double *sq, *sv;            // RK4: the state the next stage is evaluated at
  double *aq, *av;            // RK4: the weighted sums of the slopes
  const double* ddq;          // what the pass returned
  const int32_t* st_stage;    // ... and its per-sample status
  int32_t* st_run;            // running minimum; a sample below 0 gets NaN state at the last stage
  double *q_rec, *dq_rec;     // last stage, may be null: the trajectory record that is due
  int64_t count, n_samples;
  int n, element_major, integrator, stage;
  double dt;
};
hipError_t rdyn_launch_rollout_stage(const RdynRolloutStageArgs& a, hipStream_t st);
// count doubles q_src -> q_dst, dq_src -> dq_dst (a null destination is skipped); n_samples status words st_src -> st_dst (null source: 1)
struct RdynRolloutCopyArgs
{
  const double *q_src, *dq_src;
  double *q_dst, *dq_dst;
  const int32_t* st_src;
  int32_t* st_dst;
  int64_t count, n_samples;
};
hipError_t rdyn_launch_rollout_copy(const RdynRolloutCopyArgs& a, hipStream_t st);

// derivatives of the joint torque (rdyn_torque_deriv.hip): dtau/dq, dtau/dDq, M = dtau/dDDq; every output n x n per sample, element
// e = i + n k of sample s at X[s * m_ss + e * m_se]; any output may be null (not all three)
struct RdynTorqueDerivArgs
{
  const RdynChainConst* chain;           // rdyn_launch_torque_derivatives
  const RdynLongChainConst* chain_long;  // rdyn_launch_long_torque_derivatives
  const double *q, *dq, *ddq;
  int64_t n_samples, in_ss, in_sj;
  double *dtau_dq, *dtau_dv, *M;
  int64_t m_ss, m_se;
  int staged;  // doubles per record (n n): sample-major records through the wave's LDS tile (natural strides, every output line-aligned); 0 = 8-byte stores
};
hipError_t rdyn_launch_torque_derivatives(int n_joints, const RdynTorqueDerivArgs& a, hipStream_t st);
// ... of a chain with more input joints than the unrolled kernels sweep (dtau_dq, dtau_dv only; M: rdyn_launch_long_local).  The per-joint
// state of a workgroup's samples lives in LDS: rdyn_long_torque_deriv_lanes = samples per workgroup (64, 32 or 16; 0: no width fits)
int rdyn_long_torque_deriv_lanes(int n_joints);
size_t rdyn_long_torque_deriv_lds_bytes(int n_joints, int lanes);
hipError_t rdyn_launch_long_torque_derivatives(int n_joints, const RdynTorqueDerivArgs& a, hipStream_t st);

// Gram / normal equations of a column-major rows x P matrix (rdyn_gram.hip)
struct RdynGramArgs
{
  const double* A;
  const double* b;     // may be null
  int64_t rows, lda;
  int P;
  int accumulate;      // slabs += instead of slabs =
  int add_to_output;   // finish: G/c/bb += instead of =
  double* slabs;       // [blocks][NT * 256]
  double* G;
  double* c;
  double* bb;
  // Block structure of the element-major regressor image: rows [j * row_block, (j + 1) * row_block) belong to
  // input joint j and are structurally zero in columns < first_col[j] (primitives_impl.h:690-691, 1341-1347).
  // row_block == 0: no structure assumed.  Column blocks (16 wide) left of first_col[j] are neither loaded nor multiplied.
  int64_t row_block;
  int first_col[RDYN_MAX_SWEPT_JOINTS];
  // finish only: > 0 = the slabs hold the columns in the wave-pair kernel's order [tau_meas | link desc_nj - 1 | ... | link 0]
  // (rdyn_duo_gram.hip: the zero band of every row group then ends at a 16-column boundary more often); 0 = natural order
  int desc_nj;
  int desc_k;   // finish only, with desc_nj > 0: component columns in front of that order ([C | tau_meas | links descending]; P counts them)
  int group_stride;  // k_gram only: every group_stride-th 16-row group (0 / 1 = all): the subsample pass of the preconditioned route
  int slab_nb;  // finish only: 16-column blocks of the slabs' tile layout if it is wider than P + 1 columns need (0 = derive from P)
  const int* run_flag;  // finish only, may be null: device word; 0 = leave at once (conditional second round of rdyn_cholqr.hip)
  int col_shift;        // finish only: the slabs' column space is the natural order shifted right by col_shift (rdyn_cholqr.hip)
};
// normal equations of the reduced chain -> of the chain (rdyn_chain.hpp; rdyn_gram.hip: k_gram_expand)
struct RdynGramExpandArgs
{
  const double *G_red, *c_red, *bb_red;  // (10 n_red + K)^2, 10 n_red + K, 1
  const double* X;                       // device: [n_joints][10][10]
  int red_of[RDYN_MAX_JOINTS];   // per CHAIN joint (the chain may be longer than what the kernels sweep)
  int n_joints, n_red, n_comp_cols;
  int add_to_output;
  double *G, *c, *bb;                    // (10 n_joints + K)^2, 10 n_joints + K, 1 (c, bb may be null)
};
hipError_t rdyn_launch_gram_expand(const RdynGramExpandArgs& a, hipStream_t st);
hipError_t rdyn_launch_set_double(double* p, double v, hipStream_t st);  // *p = v, ordered on the stream
// fused regressor -> Gram persistent kernel (rdyn_fused_gram.hip)
struct RdynFusedGramArgs
{
  RdynSweepArgs sweep;   // chain, q/dq/ddq/bcol, n_samples, input strides (Y fields ignored)
  int n_active;
  int first_col[RDYN_MAX_SWEPT_JOINTS];
  double* images;        // [blocks][(P + 1) * n * 256] per-workgroup tile images
  double* slabs;         // [blocks][NT * 256] per-workgroup Gram slabs
  int debug;             // always 0 (no host code sets it; the phase ablation it steered is closed): the kernel's two reads stay because
                         // without them hipcc allocates every instantiation differently (CHANGELOG.md, "Retire closed experiments")
};
hipError_t rdyn_launch_regressor_gram_fused(int n_joints, const RdynFusedGramArgs& a, int blocks, hipStream_t st);

// per-joint additive components (rdyn_components.hip); constants already sanitised by the API
#define RDYN_MAX_COMPONENTS 30
struct RdynComponent
{
  int type, joint;
  double min_velocity, max_velocity;
  double parameters[3];
};
// LDS-resident regressor -> Gram / R-factor kernels (rdyn_duo_gram.hip, rdyn_cholqr.hip, rdyn_pgram_solo.hip, rdyn_tsqr*.hip): 16 samples
// per tile, packed column-major tile in LDS
struct RdynLdsGramArgs
{
  const RdynChainConst* chain;
  const double *q, *dq, *ddq, *bcol;   // bcol may be null
  int64_t n_samples, in_ss, in_sj;
  int n_active;
  // the caller's input index behind tile row r (rdyn_chain.hpp: sorted view): q, Dq, DDq, tau_meas of row r are read at in_map[r] * in_sj;
  // the identity for input joints in chain order
  int in_map[8];
  // one-lane-per-sample sweepers (rdyn_duo_gram.hip, KIN): sweep_lanes != 0 selects them (the host then sized the dynamic LDS for the
  // exchange area behind the tiles, RDYN_KIN_XCH_BYTES); sw_rows[3 (w - 1) + slot] = the tile rows sweeper wave w = 1 .. 7 computes (99 =
  // none), balanced over the waves by the cost of a row (a row of joint l is carried through the links l .. n - 1)
  int sweep_lanes;
  int sw_rows[21];
  int all_revolute;                    // every chain joint is revolute (selects the sweeper without joint-kind selects)
  int first_col[RDYN_MAX_SWEPT_JOINTS];      // per input joint: 10 * chain index
  int lds_off[RDYN_MAX_SWEPT_JOINTS];        // per link: byte offset of its first column in the tile
  int lds_stride[RDYN_MAX_SWEPT_JOINTS];     // per link: bytes between its columns = (16 m_f + 4) * 8
  int lds_m[RDYN_MAX_SWEPT_JOINTS];          // per link: number of input joints whose rows can be non-zero (stored rows = 16 m_f)
  int lds_off_b;                       // byte offset of column P (measured torque), 16 n rows
  int reserved0;                       // always 0, read by nothing: keeps the kernel-argument offsets of every kernel that takes the struct
  int tile_bytes;                      // one wave's tile
  double* slabs;
  int reserved1;                       // as reserved0
  int tile_stride;                     // wave-pair kernels: sweep every tile_stride-th 16-sample tile only (0 / 1 = all): the subsample pass of the preconditioned route
  const int* run_flag;                 // k_regressor_tsqr and its tree only: null, or a device word -- 0 = leave at once
  // wave-pair kernel only (rdyn_duo_gram.hip): the per-joint component columns [Y | C | tau_meas] of rdyn_identification_gram.
  // Column P + k of the tile belongs to component comp_col_comp[k] and is non-zero only in the rows of that component's joint:
  // it is stored as ONE 16-row group (stride 160 bytes) at lds_off_c + 160 k; the measured torque moves to column P + n_comp_cols.
  int n_comps, n_comp_cols;
  int lds_off_c, comp_stride;          // component column k at lds_off_c + comp_stride * k (160, or 144 in the compact layout)
  int col_shift;                       // k_regressor_pgram_solo only: columns of padding in front of the natural order in the consumer's column space
  int comp_row_step;                   // 0: a component column stores its own joint's 16-row group only; 128: all row groups (rectangular tile of rdyn_tsqr_wide.hip)
  signed char comp_col_row[96];        // per component column: the input joint (row group) it belongs to
  RdynComponent comps[RDYN_MAX_COMPONENTS];
};
// sweep and MFMA streams on two co-resident waves (rdyn_duo_gram.hip): chains of 2..7 joints, 512-thread workgroups
bool rdyn_regressor_gram_duo_supported(int n_cols);
// doubles per sample and exchange buffer: up to 6 joints 30 (the b-matrix too; the kernel uses 21 of them without component columns), 12 at 7
#define RDYN_KIN_XCH_BYTES(n_joints) (2 * ((n_joints) <= 6 ? 30 : 12) * 64 * 8)
#define RDYN_KIN_XCH_BYTES_XV(xv) (2 * (xv) * 64 * 8)  // (pass B of the R factor: 21 doubles per sample up to 6 joints, 12 at 7)
// the one-lane-per-sample sweepers exist for this shape: 0 no, 4 / 2 = with the standard / the compact tile layout (column padding in doubles)
int rdyn_regressor_gram_duo_kin_pad(int n_joints, int n_comp_cols);
// n_cols = 10 * chain joints; a.n_comp_cols extra component columns may add at most one 16-column block
bool rdyn_regressor_gram_duo_supports_components(int n_cols, int n_comp_cols);
hipError_t rdyn_launch_regressor_gram_duo(int n_cols, const RdynLdsGramArgs& a, int blocks, size_t lds_bytes, hipStream_t st);
// preconditioned CholeskyQR (rdyn_cholqr.hip): R factor of [A | b] with the heavy pass on the fp64 matrix cores.
//   W = R1^-1 of a Householder factor R1 of a row SUBSAMPLE (rdyn_tsqr.hip);  G2 = (A W)'(A W) over ALL rows: sweep -> LDS tile -> the
//   consumer wave multiplies every 16-row group by W (MFMA) and accumulates the Gram of the product (MFMA);  R = chol(G2) R1.
// xb = 1: one more 16-column block for the component columns of rdyn_identification_tsqr (chains of <= 6 joints)
int rdyn_cholqr_kin_pad(int n_joints, int xb, int pairs);  // pass B with the one-lane-per-sample sweepers: tile padding (4 / 2), 0 = not served
int rdyn_cholqr_pairs(int n_joints, int tile_bytes, int xb);  // 4: W in LDS beside four tiles; -4: four tiles, W in global memory; 2: two pairs on four SIMDs, -1: four waves that sweep and consume their own compact tile (7 joints + components); 0: unsupported
size_t rdyn_cholqr_w_doubles(int n_joints, int xb);           // W in MFMA operand order
// R <- qr([R ; R_new]); rows_new > 0: R_new is zero below that many rows (an expanded factor); any n1 whose packed R_new fits 156 KB of LDS
hipError_t rdyn_launch_cholqr_fold(const double* R_new, double* R, int n1, hipStream_t st, int rows_new = 0);
hipError_t rdyn_launch_regressor_pgram(int n_joints, const RdynLdsGramArgs& a, const double* W, const int* run_flag, int blocks, int pairs, hipStream_t st);
// the same pass over a materialised column-major matrix [A | b] (rdyn_tsqr): n_cols + (b != null) <= 96 columns, natural column order
hipError_t rdyn_launch_pgram_rows(const double* A, const double* b, int64_t rows, int64_t lda, int n_cols, const double* W, double* slabs,
                                  const int* run_flag, int blocks, hipStream_t st);
// R1 (n1 x n1 upper, column-major) -> T = R1 re-triangularised without its deferred columns (zmask <- that set), W = T^-1 in MFMA
// operand order.  row_scale: R1 is the factor of one row in row_scale^2 (the subsample), T is scaled to all rows.
// col_shift: columns of padding in FRONT of the natural order in the consumer's column space (rdyn_cholqr_col_shift).
// flags (device ints): [0] run round 1, [1] run the stand-by Householder factorisation, [2] run round 0.  The preconditioner of a
// round whose growth factor gamma (Q T reproduces the columns of A with a relative error of about u gamma; *gamma_out, may be null)
// exceeds 1e4 calls the round off and the stand-by in.
// V: T^-1 in natural order (n1 x n1, for the factor kernel's own evaluation of gamma).
// Input: the triangular factor R1, or (Gs != null) the Gram matrix [Gs cs; cs' bbs] of the subsample's rows (P x P, P, 1; P = n1 - 1).
// nb_w: 16-column blocks of the consumer's column space (W is written, zero-padded, for all nb_w (nb_w + 1) / 2 operand blocks)
hipError_t rdyn_launch_cholqr_precond(const double* R1, const double* Gs, const double* cs, const double* bbs, int n1, int col_shift, int nb_w,
                                      double row_scale, double* T, double* W, double* V, int* zmask, int* flags, int round, const int* run_flag,
                                      double* gamma_out, hipStream_t st, double* wide_sq = nullptr);  // wide_sq: 2 n1^2 doubles of workspace for n1 > rdyn_cholqr_max_cols_lds()
int rdyn_cholqr_max_cols();      // widest factor (right-hand side included) of the dense steps of the preconditioned route (112)
int rdyn_cholqr_max_cols_lds();  // ... with their two squares in LDS (96): what the fused regressor routes take
int rdyn_cholqr_col_shift(int n_joints, int xb);
hipError_t rdyn_launch_regressor_pgram_solo(const RdynLdsGramArgs& a, const double* W, const int* run_flag, int blocks, int pairs, hipStream_t st);  // rdyn_pgram_solo.hip
int rdyn_cholqr_solo_col_shift(int n_joints, int n_comp_cols);  // pairs == -1 at 7 joints + components (k_regressor_pgram_solo: compact tile, every wave sweeps and consumes)
// G2 = [G c; c' bb] -> R = chol(G2) T (n1 x n1 upper, column-major; zero rows at the confirmed null columns); flags[round] = 1 when the
// round is not accepted (rho_out, may be null: [0] the conditioning measure of the equilibrated Q, [2] gamma on the norms of all rows);
// round 0 clears flags[1]
hipError_t rdyn_launch_cholqr_factor(const double* G, const double* c, const double* bb, int n1, int has_b, const double* T, const double* V, const int* zmask,
                                     double* R, int* flags, int round, const int* run_flag, double* rho_out, hipStream_t st, double* wide_sq = nullptr);
// factor of the reduced chain -> factor of the chain: R = qr(R_red diag(E, I_K, 1)) (a.X, a.red_of, a.n_joints, a.n_red, a.n_comp_cols used)
hipError_t rdyn_launch_cholqr_expand(const RdynGramExpandArgs& a, const double* R_red, double* R, hipStream_t st);
size_t rdyn_cholqr_expand_lds_bytes(int n_joints, int n_red, int n_comp_cols);  // dynamic LDS of that launch (limit: 156 KB)
// the column-panel route (rdyn_tsqr_wide): the same dense steps up to rdyn_cholqr_panel_max_cols() columns, their two squares in
// wide_sq (2 n1^2 doubles of workspace), rounds 0..2 (round r > 0 started by flags[r - 1]); flags [3] n1, [4 + r] round r ran, [8 + r] not accepted
int rdyn_cholqr_panel_max_cols();
hipError_t rdyn_launch_cholqr_precond_panel(const double* R1, const double* Gs, const double* cs, const double* bbs, int n1, int nb_w, double row_scale,
                                            double* T, double* W, double* V, int* zmask, int* flags, int round, const int* run_flag,
                                            double* gamma_out, double* wide_sq, hipStream_t st);
hipError_t rdyn_launch_cholqr_factor_panel(const double* G, const double* c, const double* bb, int n1, int has_b, const double* T, const double* V,
                                           const int* zmask, double* R, int* flags, int round, const int* run_flag, double* rho_out, double* wide_sq,
                                           hipStream_t st);
hipError_t rdyn_launch_cholqr_expand_global(const RdynGramExpandArgs& a, const double* R_red, double* R, double* scratch, hipStream_t st);
hipError_t rdyn_launch_cholqr_fold_global(const double* R_new, double* R, int n1, double* scratch, hipStream_t st);
// Q = X W for an upper-triangular W in the operand order of k_cholqr_precond (nb_w = ceil(n1 / 16) blocks), 64 rows per workgroup
// (rdyn_panel_trmm.hip).  X: rows x n1 column-major ([A | b]: columns < n_cols from A (lda), column n_cols from b if b != null); Q (ldq)
// may BE A (in place, ldq == lda, b null) -- every workgroup reads its rows whole before it writes them.  The zero band of a chunk image:
// rows [j row_block, (j + 1) row_block) are zero left of column first_col[j] (row_block 0: none).
struct RdynPanelTrmmArgs
{
  const double* A;
  const double* b;
  int64_t rows, lda;
  int n_cols, n1;
  double* Q;
  int64_t ldq;
  const double* W;
  const int* run_flag;  // null, or a device word: 0 = leave at once
  int64_t row_block;
  int first_col[RDYN_MAX_JOINTS];
};
hipError_t rdyn_launch_panel_trmm(const RdynPanelTrmmArgs& a, hipStream_t st);
// the row subsample of a preconditioner: every group_stride-th 16-row group of [A | b] (b may be null) into Q (ldq >= its rows)
hipError_t rdyn_launch_panel_gather(const double* A, const double* b, int64_t rows, int64_t lda, int n_cols, int64_t group_stride, double* Q,
                                    int64_t ldq, hipStream_t st);
int64_t rdyn_panel_gather_rows(int64_t rows, int64_t group_stride);  // rows of that subsample
// tall-skinny QR (rdyn_tsqr.hip): R factor of [A | b] without forming A'A
int rdyn_tsqr_padded_cols(int n_cols_with_rhs);              // 16 / 32 / 48 / 64, 0 = unsupported
size_t rdyn_tsqr_workspace_doubles(int nc, int blocks);
int rdyn_regressor_tsqr_cols(int n_joints, int n_comp_cols);  // factor width of a rdyn_launch_regressor_tsqr call (0: unsupported)
// a.run_flag (device int, may be null): every kernel of the call leaves at once when it reads 0; tree_fan: factors folded per wave and
// tree level (2: the shallowest dependent chain; 16: three launches in all -- the stand-by call of the preconditioned route)
hipError_t rdyn_launch_regressor_tsqr(int n_joints, const RdynLdsGramArgs& a, int blocks, size_t lds_bytes, double* workspace, double* R, int accumulate,
                                      hipStream_t st, int tree_fan = 2);
hipError_t rdyn_launch_tsqr_rows(const double* A, const double* b, int64_t rows, int64_t lda, int n_cols, int blocks, double* workspace, double* R,
                                 int accumulate, hipStream_t st, const int* run_flag = nullptr, int tree_fan = 2);
// the shapes beyond the register-resident folds (rdyn_tsqr_wide.hip): factor packed in LDS, up to 112 columns
int rdyn_tsqr_wide_max_cols();
size_t rdyn_regressor_tsqr_wide_lds_bytes(int n1, int n_active);  // 0: the 16-sample tile does not fit beside the factor
size_t rdyn_tsqr_wide_workspace_doubles(int n1, int blocks);
// a: the rectangular tile layout (comp_row_step = 128); factor width 10 n_joints + a.n_comp_cols + 1; blocks <= 256; a.run_flag as above
hipError_t rdyn_launch_regressor_tsqr_wide(int n_joints, const RdynLdsGramArgs& a, int blocks, double* workspace, double* R, int accumulate, hipStream_t st);
hipError_t rdyn_launch_tsqr_wide_rows(const double* A, const double* b, int64_t rows, int64_t lda, int n_cols, int blocks, double* workspace, double* R,
                                      int accumulate, const int* run_flag, hipStream_t st);
hipError_t rdyn_launch_tsqr_fold_factors(const double* factors, int count, int64_t stride, int n1, double* scratch, double* R, int accumulate, hipStream_t st);
int rdyn_gram_blocks_for(int P);
hipError_t rdyn_launch_gram(const RdynGramArgs& a, int blocks, hipStream_t st);
hipError_t rdyn_launch_gram_finish(const RdynGramArgs& a, int blocks, hipStream_t st);

// Gram of a matrix wider than k_gram holds: column panels of RDYN_PANEL_BLOCKS 16-column blocks, one launch over every panel pair
// (rdyn_panel_gram.hip).  Same outputs as RdynGramArgs; the zero band of a regressor image may come from up to RDYN_MAX_JOINTS row blocks.
#ifndef RDYN_PANEL_BLOCKS
#define RDYN_PANEL_BLOCKS 4
#endif
struct RdynPanelGramArgs
{
  const double* A;
  const double* b;     // may be null
  int64_t rows, lda;
  int P;
  int accumulate;      // slabs += instead of slabs =
  int add_to_output;   // finish: G/c/bb += instead of =
  double* slabs;       // [pairs][blocks][RDYN_PANEL_BLOCKS^2 * 256]
  double* G;
  double* c;
  double* bb;
  // rows [j * row_block, (j + 1) * row_block) are zero in the columns < first_col[j] (any order); row_block == 0: no structure
  int64_t row_block;
  int first_col[RDYN_MAX_JOINTS];
  const int* run_flag;  // null, or a device word: 0 = both kernels leave at once (the rounds of rdyn_tsqr_wide)
};
int rdyn_panel_gram_pairs(int P);
int rdyn_panel_gram_blocks(int P);  // row-slice workgroups per pair
size_t rdyn_panel_gram_slab_bytes(int P);
hipError_t rdyn_launch_panel_gram(const RdynPanelGramArgs& a, hipStream_t st);
hipError_t rdyn_launch_panel_gram_finish(const RdynPanelGramArgs& a, hipStream_t st);

struct RdynComponentArgs
{
  const double *q, *dq;
  int64_t n_samples, in_ss, in_sj;
  int n_active, n_comps;
  double* C;            // may be null
  int64_t c_ss, c_sr, c_sc;
  double* tau;          // may be null; += component torque, same layout as q
  RdynComponent comps[RDYN_MAX_COMPONENTS];
};
hipError_t rdyn_launch_components(const RdynComponentArgs& a, hipStream_t st);

// forward dynamics and rollouts with components (rdyn_fwd_dyn_comp.hip, rdyn_rollout_comp.hip, k_fwd_solve's variant in rdyn_fwd_dyn.hip):
// the evaluation's torque is tau - tau_c(q, dq), tau_c what k_components adds to a zero-initialised tau; the table travels in the
// kernel arguments behind the arguments of the plain kernel (constants already sanitised by the API, comps[i].joint an input index)
struct RdynComponentTable
{
  int n_comps;
  RdynComponent comps[RDYN_MAX_COMPONENTS];
};
struct RdynFwdDynCompArgs
{
  RdynFwdDynArgs f;
  RdynComponentTable t;
};
hipError_t rdyn_launch_forward_dynamics_components(int n_joints, const RdynFwdDynCompArgs& a, hipStream_t st);
struct RdynFwdSolveCompArgs
{
  RdynFwdSolveArgs s;
  const double *q, *dq;  // the chunk's first sample, addressed like tau
  RdynComponentTable t;
};
hipError_t rdyn_launch_forward_solve_components(const RdynFwdSolveCompArgs& a, hipStream_t st);
// derivatives of the forward dynamics (rdyn_fwd_dyn_deriv.hip): ddq = FD_c(q, dq, tau) as rdyn_launch_forward_dynamics_components computes
// it (f.staged is not used: ddq leaves by 8-byte stores), and dddq_dq = -M^-1 (dtau_dq + d tau_c / d q), dddq_dv = -M^-1 (dtau_dv +
// d tau_c / d dq), minv = M^-1 at that ddq: n x n per sample, element e = i + n k of sample s at X[s * m_ss + e * m_se]; any matrix may be
// null (not all three)
struct RdynFwdDynDerivArgs
{
  RdynFwdDynArgs f;
  double *dddq_dq, *dddq_dv, *minv;
  int64_t m_ss, m_se;
  int staged;  // doubles per record (n n): sample-major records through the wave's LDS tile (natural strides, every matrix line-aligned); 0 = 8-byte stores
  RdynComponentTable t;
};
hipError_t rdyn_launch_forward_dynamics_derivatives(int n_joints, const RdynFwdDynDerivArgs& a, hipStream_t st);
// ... of a chain with more input joints than the unrolled kernels sweep: the chunk image holds the factor k_fwd_solve left (L in the lower
// triangle, 1 / L_jj on the diagonal); dddq_dq and dddq_dv hold dtau_dq and dtau_dv of the chunk's samples on entry and are solved in
// place, column by column; minv is written from unit columns.  status = what k_fwd_solve wrote for the chunk (not null).
struct RdynFwdSolveColumnsArgs
{
  const double* image;
  int64_t ld;
  int n;
  const int32_t* status;
  const double *q, *dq;  // the chunk's first sample
  int64_t n_samples, in_ss, in_sj;
  double *dddq_dq, *dddq_dv, *minv;
  int64_t m_ss, m_se;
  RdynComponentTable t;
};
hipError_t rdyn_launch_forward_solve_columns(const RdynFwdSolveColumnsArgs& a, hipStream_t st);
struct RdynRolloutCompArgs
{
  RdynRolloutArgs r;
  RdynComponentTable t;
};
hipError_t rdyn_launch_rollout_components(int n_joints, const RdynRolloutCompArgs& a, hipStream_t st);

// forward dynamics and rollouts with external link wrenches (rdyn_fwd_dyn_ext.hip, rdyn_rollout_ext.hip): the evaluation's torque is
// tau - tau_c(q, dq) - tau_E(q, ext), tau_E the joint torque of the wrenches alone (rdyn_joint_torque_ext's convention).  The wrenches
// enter the net wrench of their link inside the evaluation; the arguments travel behind those of the kernel with components.
struct RdynExtArgs
{
  const double* w;  // element e of sample s of step t at w[t * step + s * ss + e * se]
  int64_t ss, se;
  int64_t step;     // rollouts: doubles between the wrenches of consecutive steps (0: the same at every step)
  int one;          // 0: links x 6 per sample, every chain link; 1 + l: 6 per sample, applied to chain link l alone
};
struct RdynFwdDynExtArgs
{
  RdynFwdDynCompArgs c;
  RdynExtArgs x;
};
hipError_t rdyn_launch_forward_dynamics_ext(int n_joints, const RdynFwdDynExtArgs& a, hipStream_t st);
struct RdynRolloutExtArgs
{
  RdynRolloutCompArgs c;
  RdynExtArgs x;
};
hipError_t rdyn_launch_rollout_ext(int n_joints, const RdynRolloutExtArgs& a, hipStream_t st);

// closed-loop rollouts (rdyn_rollout_fb.hip): the evaluation's actuator torque is the command of a joint-space PD law,
//     u = fma(kd, dq_ref - dq, fma(kp, q_ref - q, tau_ff)),  then clamped to +-lim by comparisons (a NaN command stays NaN),
// tau_ff the torque sequence of RdynRolloutArgs; components and wrenches are applied behind the clamp.  Every array is in input order.
struct RdynFeedbackArgs
{
  const double *q_ref, *dq_ref;  // step t at + t * ref_step, addressed like q; dq_ref null: zero
  int64_t ref_step;              // doubles between the references of consecutive steps (0: a constant set point)
  const double *kp, *kd;         // per_sample 0: n values shared by all samples; 1: addressed like q.  kd null: no velocity term
  const double* lim;             // n values, may be null: no clamp
  double* tau_traj;              // may be null: record k = the command of the first evaluation of step (k + 1) traj_every - 1, at + k * traj_step
  int per_sample, hold;          // hold 1: the command of the step's first evaluation serves the whole step; 0: formed at every stage
};
struct RdynRolloutFbArgs
{
  RdynRolloutExtArgs e;  // e.x.w null: no wrenches (the kernels without the wrench path)
  RdynFeedbackArgs f;
};
hipError_t rdyn_launch_rollout_feedback(int n_joints, const RdynRolloutFbArgs& a, hipStream_t st);
// ... of a chain on the chunked route: the command of one evaluation, one thread per double of the (contiguous) arrays in the batch's
// layout.  q, dq = the state the evaluation runs at; tau_ff, q_ref, dq_ref = the step's; u = the workspace array the pass takes as its
// torques; rec = the command record that is due (null: none; a sample whose running status is below 0 gets quiet NaN).
struct RdynRolloutCommandArgs
{
  const double *q, *dq, *tau_ff, *q_ref, *dq_ref, *kp, *kd, *lim;
  double *u, *rec;
  const int32_t* st_run;
  int64_t count, n_samples;
  int n, element_major, per_sample;
};
hipError_t rdyn_launch_rollout_command(const RdynRolloutCommandArgs& a, hipStream_t st);

// closed-loop rollouts under a model-based law (rdyn_rollout_fb_model.hip, rdyn_model_law.h): the controller's model is swept at every
// evaluation whose command is formed; chains swept in registers only.  With tau_m = RNEA_model (rdyn_joint_torque of the model chain):
//   RDYN_LAW_COMPUTED_TORQUE        a = fma(kd, dq_ref - dq, fma(kp, q_ref - q, ddq_ref)),  u = clamp(tau_ff + tau_m(q, dq, a))
//   RDYN_LAW_GRAVITY_COMPENSATION   u = clamp(fma(kd, dq_ref - dq, fma(kp, q_ref - q, tau_ff)) + tau_m(q, 0, 0))
struct RdynModelFeedbackArgs
{
  const RdynChainConst* model;  // device pointer: the constants of the model chain that is swept (the same joints and input joints as the plant's)
  const double* ddq_ref;        // computed torque, may be null (zero): step t at + t * ref_step of RdynFeedbackArgs, addressed like q
  int law;                      // rdyn_feedback_law
};
struct RdynRolloutModelFbArgs
{
  RdynRolloutFbArgs b;
  RdynModelFeedbackArgs m;
};
hipError_t rdyn_launch_rollout_model_feedback(int n_joints, const RdynRolloutModelFbArgs& a, hipStream_t st);

// reverse-mode product of the forward dynamics (rdyn_fwd_dyn_vjp.hip): with ddq = FD_c(q, dq, tau) and the seed ddq_bar per sample,
// tau_bar = M^-1 ddq_bar, q_bar = dddq_dq' ddq_bar, dq_bar = dddq_dv' ddq_bar (the matrices of RdynFwdDynDerivArgs).  Every vector is
// addressed like q; any output may be null (not all three of the products); tau_bar may alias ddq_bar.
struct RdynFwdDynVjpArgs
{
  const RdynChainConst* chain;
  const double *q, *dq, *tau, *ddq_bar;
  double *q_bar, *dq_bar, *tau_bar, *ddq;
  int32_t* status;  // may be null: 1, or -1 (a pivot failed or an input of the sample is not finite: every output of the sample is NaN)
  int64_t n_samples, in_ss, in_sj;
  int staged;       // doubles per record (n_active): sample-major records through the wave's LDS tile (natural strides, every output line-aligned); 0 = 8-byte stores
  RdynComponentTable t;
};
hipError_t rdyn_launch_forward_dynamics_vjp(int n_joints, const RdynFwdDynVjpArgs& a, hipStream_t st);
// ... with respect to the parameters (rdyn_fwd_dyn_param_vjp.hip): pi_bar = -Y(q, dq, ddq)' w, comp_bar = -C(q, dq)' w with
// w = tau_bar = M^-1 ddq_bar.  v = the arguments of the product above (q_bar, dq_bar are not used); the swept chain has n_joints links.
// Rows: column k of sample s at pi_bar[s * pi_ss + k * pi_sc] (10 n_full columns) and comp_bar[s * comp_ss + k * comp_sc]
// (n_comp_cols columns); partials: [waves][10 n_joints + n_comp_cols], the sums of each wave's samples, the swept chain's columns.
// expand: null, or the blocks X_f of the chain of n_full joints the swept chain is the companion of, red_of its link -> body map.
struct RdynFwdDynParamVjpArgs
{
  RdynFwdDynVjpArgs v;
  double *pi_bar, *comp_bar;  // may be null
  int64_t pi_ss, pi_sc, comp_ss, comp_sc;
  double* partials;           // may be null
  int n_comp_cols;
  const double* expand;
  int n_full;
  int red_of[RDYN_MAX_JOINTS];  // (ints: RdynSweepArgs::expand_red_of says why)
};
hipError_t rdyn_launch_forward_dynamics_parameter_vjp(int n_joints, const RdynFwdDynParamVjpArgs& a, hipStream_t st);
// S[col] = the sum over r < n_rows of x[r * row_stride + col * col_stride], col < 10 n_swept + n_comp_cols, the rows whose status word is
// not 1 left out (status null: none) -> pi_sum[10 n_full], comp_sum[n_comp_cols] (each may be null; accumulate: += instead of =),
// through expand / red_of as above (null: n_full = n_swept).  S is workspace.  Two launches, fixed order of additions.
struct RdynParamSumArgs
{
  const double* S;
  double *pi_sum, *comp_sum;
  int accumulate, n_swept, n_full, n_comp_cols;
  const double* expand;
  int red_of[RDYN_MAX_JOINTS];  // (ints: RdynSweepArgs::expand_red_of says why)
};
hipError_t rdyn_launch_parameter_sums(const double* x, int64_t n_rows, int64_t row_stride, int64_t col_stride, const int32_t* status,
                                      const RdynParamSumArgs& a, hipStream_t st);
// ... its two halves: S[col] of `cols` columns alone, and S -> the caller's vectors
hipError_t rdyn_launch_parameter_column_sums(const double* x, int64_t n_rows, int64_t row_stride, int64_t col_stride, const int32_t* status,
                                             int cols, double* S, hipStream_t st);
hipError_t rdyn_launch_parameter_sums_finish(const RdynParamSumArgs& a, hipStream_t st);
// ... of a chain with more input joints than the unrolled kernels sweep: the rows of one chunk from its element-major image [Y (P) | C (K)]
// (row j * cnt + s, column stride lda) and tau_bar / status of the chunk's samples (pointers at the chunk's first sample, tau_bar
// addressed like q): row[col] = -sum_j image(j, s, col) tau_bar_j, quiet NaN where status is not 1.  pi_rows / comp_rows may be null.
struct RdynParamProductArgs
{
  const double* image;
  int64_t cnt, lda;
  int n, P, K;
  const double* tau_bar;
  int64_t in_ss, in_sj;
  const int32_t* status;
  double *pi_rows, *comp_rows;
  int64_t pi_ss, pi_sc, comp_ss, comp_sc;
};
hipError_t rdyn_launch_parameter_rows_from_image(const RdynParamProductArgs& a, hipStream_t st);
// ... of a chain with more input joints than the unrolled kernels sweep: the three transposed products from the matrices
// rdyn_forward_dynamics_derivatives left element-major in the workspace (element e = i + n k of sample s of the chunk at X[e * ld + s]);
// status = what that call wrote for the chunk (not null)
struct RdynVjpProductArgs
{
  const double *dddq_dq, *dddq_dv, *minv;  // dddq_dq / dddq_dv may be null with q_bar / dq_bar
  int64_t ld;
  int n;
  const double *q, *dq, *tau, *ddq_bar;  // the chunk's first sample: a sample with a non-finite entry gets -1
  int64_t seed_ss, seed_sj;              // ... of ddq_bar (the host hands over a copy: tau_bar may alias the caller's)
  double *q_bar, *dq_bar, *tau_bar;
  double* ddq;          // may be null: gets NaN where the sample fails here
  int32_t* status;      // the chunk's, read and updated
  int32_t* status_out;  // may be null: the caller's
  int64_t n_samples, in_ss, in_sj;
};
hipError_t rdyn_launch_vjp_products(const RdynVjpProductArgs& a, hipStream_t st);
// dst[i * ld + s] = src[s * in_ss + i * in_sj], i < n, s < n_samples: the chunk's seeds into the workspace
hipError_t rdyn_launch_vjp_seed_copy(const double* src, double* dst, int n, int64_t n_samples, int64_t ld, int64_t in_ss, int64_t in_sj, hipStream_t st);

// adjoint of a rollout (rdyn_rollout_adjoint.hip): the transpose of the T steps RdynRolloutArgs describes, backwards from the seeds on the
// end state (and on every trajectory record) to the gradients with respect to the initial state and the torques
struct RdynRolloutAdjointArgs
{
  const RdynChainConst* chain;
  const double *q, *dq, *tau;          // x_0 and the forward call's torques
  int64_t tau_step;
  const double *q_traj, *dq_traj;      // record k = x_{k + 1}
  int64_t traj_step;
  const double *gq_end, *gdq_end;      // may be null (0)
  const double *gq_traj, *gdq_traj;    // may be null: record k = the seed on x_{k + 1}
  int64_t gtraj_step;
  double *gq0, *gdq0;                  // may be null; may alias gq_end / gdq_end
  double* gtau;                        // may be null
  int64_t gtau_step;                   // 0: the sum over the steps
  int32_t* status;                     // may be null
  int64_t n_samples, in_ss, in_sj;
  double dt;
  int n_steps, integrator, n_active;
  int staged;  // sample-major records through the wave's LDS tile in whole lines: bit 0 gq0 / gdq0, bit 1 gtau
  RdynComponentTable t;
};
hipError_t rdyn_launch_rollout_adjoint(int n_joints, const RdynRolloutAdjointArgs& a, hipStream_t st);
// ... with the gradients with respect to the parameters (rdyn_rollout_adjoint_params.hip, one object per integrator): the same sweep, and
// every product adds its rows to acc[col * ld + s] (10 n_joints + n_comp_cols columns, zeroed by the kernel), status[s] = the sample's
// final verdict; rdyn_launch_parameter_sums(acc, n_samples, 1, ld, status, ...) makes the sums of them
hipError_t rdyn_launch_rollout_adjoint_params_euler(int n_joints, const RdynRolloutAdjointArgs& a, double* acc, int64_t ld, int32_t* status,
                                                    int n_comp_cols, hipStream_t st);
hipError_t rdyn_launch_rollout_adjoint_params_rk4(int n_joints, const RdynRolloutAdjointArgs& a, double* acc, int64_t ld, int32_t* status,
                                                  int n_comp_cols, hipStream_t st);
// ... of a chain with more input joints than the unrolled kernels sweep: the element-wise updates between the passes of the host loop
// (rdyn_api_dynamics.cpp).  Every array holds count = n * n_samples doubles in the batch's layout; op selects the update (the formulas are at the
// head of rdyn_rollout_adjoint.hip).
enum
{
  RDYN_ADJ_OP_INIT = 0,        // lq = a + b, lv = c + d (null = 0); st_run = 1
  RDYN_ADJ_OP_EULER_PRE = 1,   // lv = lv + dt lq; mv = dt lv (the seed of the product)
  RDYN_ADJ_OP_EULER_POST = 2,  // lq += qb, lv += vb, gtau (= | +=) tb; st_run = min(st_run, st_stage); NaN for a failed sample
  RDYN_ADJ_OP_RK4_FWD = 3,     // sq = a + cdt c, sv = b + cdt d: the next stage state from x_t = (a, b), the stage velocity c and acceleration d
  RDYN_ADJ_OP_RK4_PRE = 4,     // xq = lq, xv = lv, kq = kv = mq = 0
  RDYN_ADJ_OP_RK4_SEED = 5,    // kq = dt wgt lq + kq, mv = dt wgt lv + kv (the seed of the product)
  RDYN_ADJ_OP_RK4_POST = 6,    // mq += tb, xq += qb, xv += kq + vb, (kq, kv) = cdt (qb, kq + vb); st_run = min(st_run, st_stage)
  RDYN_ADJ_OP_RK4_END = 7,     // lq = xq, lv = xv, gtau (= | +=) mq; NaN for a failed sample
  RDYN_ADJ_OP_ADD_SEED = 8,    // lq += a, lv += b (null = 0): the running seeds that are due
  RDYN_ADJ_OP_OUT = 9,         // lq -> out_q, lv -> out_v, st_run -> status (each may be null)
  RDYN_ADJ_OP_ZERO = 10        // gtau = 0
};
struct RdynAdjointUpdateArgs
{
  int op;
  double *lq, *lv;              // the adjoint state
  double *xq, *xv;              // RK4: x_bar
  double *kq, *kv;              // RK4: the carry into the next-lower stage's seed, then that stage's kq
  double *mq, *mv;              // RK4: the step's torque gradient; the seed handed to the product
  const double *qb, *vb, *tb;   // what the product returned
  const double *a, *b, *c, *d;  // op-specific inputs
  double *sq, *sv;              // RDYN_ADJ_OP_RK4_FWD: the next stage's state
  double *out_q, *out_v;        // RDYN_ADJ_OP_OUT
  double* gtau;                 // may be null
  int gtau_add;                 // gtau += instead of =
  const int32_t* st_stage;      // the product's status
  int32_t* st_run;              // the running minimum
  int32_t* status;              // RDYN_ADJ_OP_OUT
  int64_t count, n_samples;
  int n, element_major;
  double dt, wgt, cdt;          // b_i and c_i of the stage
};
hipError_t rdyn_launch_adjoint_update(const RdynAdjointUpdateArgs& a, hipStream_t st);

// the product and the adjoint with external link wrenches (rdyn_fwd_dyn_vjp_ext.hip, rdyn_rollout_adjoint_ext.hip): of
// ddq = FD_c(q, dq, tau - tau_E(q, ext)) and of the rollout RdynRolloutExtArgs describes.  x = the wrenches (w not null); ext_bar / gw: null,
// or -(d tau_E / d ext)' w in the layout of x.w (strides x.ss, x.se), step t of the adjoint at gw + t * gw_step (0: the sum over the steps).
struct RdynFwdDynVjpExtArgs
{
  RdynFwdDynVjpArgs v;
  RdynExtArgs x;
  double* ext_bar;
};
hipError_t rdyn_launch_forward_dynamics_vjp_ext(int n_joints, const RdynFwdDynVjpExtArgs& a, hipStream_t st);
struct RdynRolloutAdjointExtArgs
{
  RdynRolloutAdjointArgs a;
  RdynExtArgs x;
  double* gw;
  int64_t gw_step;
};
hipError_t rdyn_launch_rollout_adjoint_ext_euler(int n_joints, const RdynRolloutAdjointExtArgs& a, hipStream_t st);
hipError_t rdyn_launch_rollout_adjoint_ext_rk4(int n_joints, const RdynRolloutAdjointExtArgs& a, hipStream_t st);

// the adjoint of a closed-loop rollout (rdyn_rollout_adjoint_fb.hip): of the rollout RdynRolloutFbArgs describes.  ax = the adjoint's
// arguments (ax.x.w null: no wrenches, ax.gw null then; ax.a.gtau is the gradient with respect to the feed-forward torques), f = the
// forward call's law (tau_traj is not read), g = where the law's gradients go.  Every array of g is addressed like q.
struct RdynFeedbackGradArgs
{
  double *gq_ref, *gdq_ref;   // may be null: step t at + t * gref_step
  int64_t gref_step;          // 0: one record, the sum over the steps
  double *gkp, *gkd, *glim;   // may be null: one row per SAMPLE, summed over the steps
  const double* gu;           // may be null: record t = the seed on the command of step t's first evaluation, at + t * gu_step
  int64_t gu_step;
  int accumulate;             // 1: gkp, gkd, glim and the gref_step = 0 sums continue from what is there
  int staged;                 // the per-step records of gq_ref / gdq_ref leave through the wave's LDS tile in whole lines
};
struct RdynRolloutAdjointFbArgs
{
  RdynRolloutAdjointExtArgs ax;
  RdynFeedbackArgs f;
  RdynFeedbackGradArgs g;
};
hipError_t rdyn_launch_rollout_adjoint_feedback(int n_joints, const RdynRolloutAdjointFbArgs& a, hipStream_t st);
// ... with the gradients with respect to the parameters (rdyn_rollout_adjoint_fb_params.hip, one object per integrator; a.ax.x.w null): the
// same sweep, and every product adds its rows to acc[col * ld + s] as rdyn_launch_rollout_adjoint_params_* does
hipError_t rdyn_launch_rollout_adjoint_feedback_params_euler(int n_joints, const RdynRolloutAdjointFbArgs& a, double* acc, int64_t ld,
                                                             int32_t* status, int n_comp_cols, hipStream_t st);
hipError_t rdyn_launch_rollout_adjoint_feedback_params_rk4(int n_joints, const RdynRolloutAdjointFbArgs& a, double* acc, int64_t ld, int32_t* status,
                                                           int n_comp_cols, hipStream_t st);

// pieces of rdyn_identification_tsqr for the multi-device form (rdyn_api_tsqr.cpp): widths of the swept / the chain's factor, the factor of
// the swept chain alone, the expansion (+ accumulation) of a swept factor
int rdyn_internal_tsqr_widths(const rdyn_chain* c, const rdyn_component* comps, int n_comps, int* n1s, int* n1, int* expands);
int rdyn_internal_tsqr_swept(const rdyn_chain* c, const rdyn_component* comps, int n_comps, const rdyn_batch* b, const double* tau_meas, double* R_swept,
                             void* workspace, size_t workspace_bytes);
int rdyn_internal_tsqr_expand(const rdyn_chain* c, const rdyn_component* comps, int n_comps, const double* R_swept, double* R, int accumulate,
                              double* scratch, void* stream);
// y[i] += x[i], i < n, ordered on the stream (rdyn_gram.hip)
hipError_t rdyn_launch_add_doubles(double* y, const double* x, int64_t n, hipStream_t st);

// every getter of a sample in one launch (rdyn_kernels.hip: k_sample_all): the argument blocks of the single-purpose kernels, one per role;
// a role whose outputs are all null leaves at once
struct RdynAllArgs
{
  int64_t n_samples;
  RdynKinArgs frames, jacobian, twists;
  RdynSweepArgs torque, torque_nl, inertia, regressor;
};
hipError_t rdyn_launch_sample_all(int n_joints, const RdynAllArgs& a, hipStream_t st);

enum { RDYN_MODE_REGRESSOR = 0, RDYN_MODE_TORQUE = 1, RDYN_MODE_INERTIA = 2, RDYN_MODE_REGRESSOR_GRAM = 3, RDYN_MODE_REGRESSOR_EXPAND = 4,
       RDYN_MODE_REGRESSOR_EXPAND_STAGED = 5 };

hipError_t rdyn_launch_local_sweep(int n_joints, int mode, const RdynSweepArgs& a, hipStream_t st);
hipError_t rdyn_launch_base_sweep(int n_joints, const RdynKinArgs& a, hipStream_t st);
hipError_t rdyn_launch_rowpair_sweep(int n_joints, int n_active, const RdynSweepArgs& a, hipStream_t st);
// per-sample Eigen image (y_sr == 1, y_sc == n_active) and stacked matrix (y_ss == n_active): one thread per sample, link blocks staged
// through LDS and written in whole lines (rdyn_image.hip / rdyn_image_impl.h).  fix_mask: bit f set = chain joint f is not an input
// joint; the input joints are the others, in chain order.  Compiled patterns: <= 1 fixed head joint, <= 3 fixed tail joints.
bool rdyn_image_supported(int n_joints, unsigned fix_mask, int64_t y_ss, bool multi);
hipError_t rdyn_launch_image_sweep(int n_joints, unsigned fix_mask, const RdynSweepArgs& a, hipStream_t st, int mapped = 0);  // mapped: 1 = run-time row map, 2 = + expansion to a longer chain
bool rdyn_image_expand_supported(int n_red, int n_full, int64_t y_ss);
bool rdyn_image_map_supported(int n_joints, unsigned fix_mask, int64_t y_ss);  // per-sample images through a run-time row map (any input order, fixed joints anywhere)
hipError_t rdyn_launch_image_sweep_multi(int n_joints, unsigned fix_mask, bool stacked, const RdynSweepArgs* table, int n_items, int64_t max_samples,
                                         hipStream_t st);  // 2..8 input joints
hipError_t rdyn_launch_local_sweep_multi(int n_joints, int mode, const RdynSweepArgs* table, int n_items, int64_t max_samples, hipStream_t st);

#endif
