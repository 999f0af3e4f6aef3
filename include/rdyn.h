/*
 * rdyn.h -- C-ABI of librdyn_hip.so: batched rigid-body dynamics of a serial chain on AMD MI355X (gfx950).
 *
 * Drop-in boundary for ONE path of CNR-STIIMA-IRAS/rosdyn: the public surface of `class rosdyn::Chain`
 * (rosdyn_core/include/rosdyn_core/primitives.h:235-555) restricted to
 *   getTransformation(s) / getJacobian / getTwist / getDTwist / getJointTorque /
 *   getJointTorqueNonLinearPart / getRegressor / getJointInertia / getNominalParameters,
 * evaluated for N samples (q, Dq, DDq) per call instead of one.  The reference has no FFI layer; a
 * maintainer binds these symbols from `rosdyn::Chain` (see INTEGRATION.md, and the ready-made C++
 * facade rosdyn_amd/csrc/rosdyn_chain_facade.hpp which keeps the reference's method names).
 *
 * Contract = the STATELESS function (chain, q, Dq, DDq) -> outputs that a freshly constructed reference
 * Chain computes on its first call (the reference's value caches, primitives_impl.h:886/985/1088, are
 * not reproduced).  All arithmetic is IEEE fp64.  Conventions are the reference's: spatial vectors are
 * [linear; angular] (spacevect_algebra.h:44-52); twists/Jacobians are expressed in the base frame with
 * the link's own origin as reference point; the regressor has 10 columns per chain joint INCLUDING fixed
 * joints, parameter order [m, m cx, m cy, m cz, Ixx, Ixy, Ixz, Iyy, Iyz, Izz] with the inertia taken
 * about the link origin (primitives_impl.h:399-417, 1295-1355); rows exist only for the active (input)
 * joints, in input order (primitives_impl.h:1352).
 *
 * Memory: every `const double*` / `double*` in a batched call is a DEVICE pointer (hipMalloc or a
 * torch.cuda tensor's data_ptr()).  Nothing is copied to or from the host, no allocation and no
 * synchronisation happens inside a batched call (graph-capturable) except the one-time upload of a
 * chain's constants (~4 KB) the first time a chain is used on a device.
 *
 * Error handling: every function returns an rdyn_status; rdyn_last_error() returns the thread-local
 * message.  Where the reference throws (std::runtime_error("Base link not found") primitives_impl.h:603,
 * "Tool link not found" :610, std::invalid_argument("Input data dimensions mismatch") :1302) the same
 * text is the message and the facade re-throws the same exception types.
 */
#ifndef RDYN_H
#define RDYN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RDYN_VERSION 100
/* Chain joints INCLUDING fixed ones (reference: m_joints_number, primitives_impl.h:638).  The reference's default build is
 * unbounded (rosdyn_core/CMakeLists.txt:12-16: MAX_NUM_AXES = -1); here a chain may have up to RDYN_MAX_JOINTS joints.
 *  - Chains of up to RDYN_MAX_SWEPT_JOINTS joints: kernels instantiated per joint count, every per-link quantity in registers.
 *  - Longer chains (long because of FIXED frames as a rule: a tool changer, a camera mount, the flange / tool0 frames of the public
 *    UR and Panda models), input joints listed in ANY order (setInputJointsName, primitives_impl.h:705-737):
 *      the by-link kinematic outputs -- rdyn_transformation, rdyn_jacobian(_link), rdyn_twist, rdyn_twist_parts, rdyn_jerk_parts,
 *      rdyn_wrench, rdyn_joint_torque_ext -- run on kernels with a run-time link loop (rdyn_long_kin.hip), any number of input joints;
 *      rdyn_regressor, rdyn_joint_torque(_nonlinear), rdyn_joint_inertia, rdyn_nominal_parameters, the normal equations, the R factors
 *      and rdyn_local_ik sweep the REDUCED COMPANION -- the input joints (at most RDYN_MAX_SWEPT_JOINTS) with the fixed frames folded
 *      into the neighbouring bodies, rdyn_chain_reduction -- and restore the columns of every folded link exactly (Y_f = Y_body X_f);
 *      with MORE input joints than that (up to RDYN_MAX_JOINTS of them; rdyn_long_local.hip: rolled link and row loops, the per-joint
 *      state in wave-private LDS) rdyn_regressor (+ its fused torque), rdyn_joint_inertia, the joint torques (read off the wrench
 *      recursion) and every kinematic output are served, rdyn_regressor_gram and rdyn_regressor_tsqr for 11 input joints (110 + 1 columns:
 *      what the Gram kernel and the widest R factor hold; chunk images; wider: the _wide calls below) and rdyn_local_ik(_damped)
 *      (rdyn_long_ik.hip: up to RDYN_MAX_JOINTS input joints; see rdyn_local_ik_damped for its undamped and negative-weight cases).
 *  - Normal equations: rdyn_gram, rdyn_regressor_gram and rdyn_identification_gram stop at 111 columns (110 + tau_meas, after the
 *    reduction); rdyn_gram_wide, rdyn_regressor_gram_wide and rdyn_identification_gram_wide serve the rest up to
 *    RDYN_MAX_WIDE_COLUMNS columns (any chain above, components included).  The R factors: rdyn_tsqr, rdyn_regressor_tsqr and
 *    rdyn_identification_tsqr stop at 112 columns with the rhs; rdyn_tsqr_wide, rdyn_regressor_tsqr_wide and
 *    rdyn_identification_tsqr_wide serve up to RDYN_MAX_WIDE_COLUMNS + 1 columns with the rhs. */
#define RDYN_MAX_JOINTS 32
#define RDYN_MAX_SWEPT_JOINTS 10

typedef enum rdyn_status
{
  RDYN_OK = 0,
  RDYN_ERR_INVALID_ARGUMENT = 1, /* NULL pointers, negative sizes, dimension mismatch                    */
  RDYN_ERR_BASE_NOT_FOUND = 2,   /* "Base link not found"   primitives_impl.h:603                        */
  RDYN_ERR_TOOL_NOT_FOUND = 3,   /* "Tool link not found"   primitives_impl.h:610                        */
  RDYN_ERR_URDF = 4,             /* malformed URDF XML                                                   */
  RDYN_ERR_UNSUPPORTED = 5,      /* more than RDYN_MAX_JOINTS chain joints, or a shape an entry point does not serve */
  RDYN_ERR_JOINT_NOT_FOUND = 6,  /* setInputJointsName: "Joint named '%s' not found" primitives_impl.h:734 */
  RDYN_ERR_NO_DEVICE = 7,        /* no HIP device / HIP runtime failure at start-up                      */
  RDYN_ERR_HIP = 8               /* a HIP call failed (message carries hipGetErrorString)                */
} rdyn_status;

/* rosdyn::Joint::Type, primitives.h:67 (same numeric values) */
typedef enum rdyn_joint_type { RDYN_REVOLUTE = 0, RDYN_PRISMATIC = 1, RDYN_FIXED = 2 } rdyn_joint_type;

/* urdf::Joint::type values as urdfdom defines them; mapped by primitives_impl.h:74-83:
 * revolute|continuous -> REVOLUTE, prismatic -> PRISMATIC, everything else -> FIXED */
typedef enum rdyn_urdf_joint_type
{
  RDYN_URDF_UNKNOWN = 0, RDYN_URDF_REVOLUTE = 1, RDYN_URDF_CONTINUOUS = 2, RDYN_URDF_PRISMATIC = 3,
  RDYN_URDF_FLOATING = 4, RDYN_URDF_PLANAR = 5, RDYN_URDF_FIXED = 6
} rdyn_urdf_joint_type;

typedef struct rdyn_chain rdyn_chain; /* opaque; immutable after creation except rdyn_chain_set_input_joints */

/* ---- flat POD description of one serial chain, base -> tool (what Chain::init extracts from the urdf tree,
 *      primitives_impl.h:600-636).  For callers that already hold a parsed urdf::Model. ------------------- */
typedef struct rdyn_joint_desc
{
  char name[64];
  int32_t urdf_type;         /* rdyn_urdf_joint_type */
  double origin_xyz[3];      /* parent_to_joint_origin_transform.position            (primitives_impl.h:54) */
  double origin_quat[4];     /* parent_to_joint_origin_transform.rotation  x,y,z,w   (urdf_parser.h:44-50)  */
  double axis[3];            /* urdf joint axis, not necessarily normalised          (primitives_impl.h:55-59) */
  int32_t has_limits;        /* urdf_joint->limits != NULL                           (primitives_impl.h:87)  */
  double lower, upper, velocity, effort;
} rdyn_joint_desc;

typedef struct rdyn_link_desc
{
  char name[64];
  int32_t has_inertial;      /* urdf_link->inertial != NULL                          (primitives_impl.h:291) */
  double mass;
  double com_xyz[3];         /* inertial->origin.position                            (primitives_impl.h:305-307) */
  double com_quat[4];        /* inertial->origin.rotation x,y,z,w                    (primitives_impl.h:309-314) */
  double ixx, ixy, ixz, iyy, iyz, izz;
} rdyn_link_desc;

typedef struct rdyn_chain_desc
{
  int32_t n_joints;                  /* chain joints incl. fixed; links = n_joints + 1 */
  const rdyn_joint_desc* joints;     /* [n_joints], joint i connects links[i] -> links[i+1] */
  const rdyn_link_desc* links;       /* [n_joints + 1], links[0] = base link */
  double gravity[3];                 /* base-frame gravity vector; the reference's default is zero (primitives.h:346) */
} rdyn_chain_desc;

/* ---- construction (host only) --------------------------------------------------------------------- */
/* rosdyn::createChain(urdf::ModelInterface, base, tool, gravity)  primitives.h:566, primitives_impl.h:1518.
 * urdf_xml is the robot_description string; a minimal reader reproduces the urdfdom behaviour the
 * reference relies on (rpy->quaternion, default axis (1,0,0), missing origin/inertial). */
int rdyn_chain_from_urdf(const char* urdf_xml, const char* base_link, const char* tool_link,
                         const double gravity[3], rdyn_chain** out);
int rdyn_chain_from_desc(const rdyn_chain_desc* desc, rdyn_chain** out);
/* Chain::clone() primitives_impl.h:552 -- an independent deep copy */
int rdyn_chain_clone(const rdyn_chain* chain, rdyn_chain** out);
/* The chain with other inertial parameters (no reference counterpart: what an identification loop needs to try its next iterate).
 * pi holds 10 * rdyn_chain_joints_number doubles (HOST pointer) in the order and convention of rdyn_nominal_parameters:
 * [m, m c, Ixx Ixy Ixz Iyy Iyz Izz about the link origin] per child link.  *out is an independent chain equal to
 * rdyn_chain_clone(chain) in everything else -- joints, limits, gravity, the base link, the current input-joint selection and order --
 * with its own reduced companion, sorted view and expansion blocks; no device copy is shared and `chain` is not touched.
 * The parameters are STORED AS GIVEN, not converted to a link description: rdyn_nominal_parameters of the new chain returns the very
 * bits of pi, and a massless link with a first moment or an inertia (which rdyn_link_desc cannot express) is accepted.
 * rdyn_chain_link_parameters then reports mass = pi[0] and cog = (m c) / m, the link origin for a massless link.
 * Physical consistency (positive mass, positive-definite inertia) is not checked: the dynamics calls report -1 per sample where M is not
 * positive definite.  A NULL argument or an entry that is not finite is RDYN_ERR_INVALID_ARGUMENT (the message names the link). */
int rdyn_chain_with_parameters(const rdyn_chain* chain, const double* pi, rdyn_chain** out);
void rdyn_chain_destroy(rdyn_chain* chain);
const char* rdyn_last_error(void);

/* ---- introspection (host only); reference getters primitives.h:364-447 ------------------------------ */
int rdyn_chain_links_number(const rdyn_chain* chain);          /* getLinksNumber        */
int rdyn_chain_joints_number(const rdyn_chain* chain);         /* getJointsNumber       */
int rdyn_chain_active_joints_number(const rdyn_chain* chain);  /* getActiveJointsNumber */
int rdyn_chain_moveable_joints_number(const rdyn_chain* chain);
const char* rdyn_chain_link_name(const rdyn_chain* chain, int i);            /* getLinksName().at(i)          */
const char* rdyn_chain_joint_name(const rdyn_chain* chain, int i);           /* chain order, incl. fixed      */
const char* rdyn_chain_moveable_joint_name(const rdyn_chain* chain, int i);  /* getMoveableJointName(i)       */
const char* rdyn_chain_active_joint_name(const rdyn_chain* chain, int i);    /* getActiveJointName(i)         */
int rdyn_chain_joint_type(const rdyn_chain* chain, int i);                   /* rdyn_joint_type of chain joint i */
int rdyn_chain_gravity(const rdyn_chain* chain, double gravity[3]);          /* getGravity                    */
/* Chain::setInputJointsName primitives_impl.h:705.  Unknown names -> RDYN_ERR_JOINT_NOT_FOUND and the
 * chain is left unchanged (the reference returns false and continues in an inconsistent state). */
int rdyn_chain_set_input_joints(rdyn_chain* chain, const char* const* names, int n_names);
/* getQMax/getQMin/getDQMax/getDDQMax/getTauMax of the active joints (primitives_impl.h:85-143, 768-776);
 * any pointer may be NULL */
int rdyn_chain_limits(const rdyn_chain* chain, double* q_max, double* q_min, double* dq_max, double* ddq_max, double* tau_max);
/* The object tree behind a reference Chain (getJoints() / getLinks(), primitives.h:62-232), read only.
 * Chain joint i (chain order, fixed joints included): R_pj row-major 3x3 and t_pj of parent <- joint (primitives_impl.h:54, 68), the
 * normalised axis in the joint frame (:55-59), limits = {q_max, q_min, Dq_max, DDq_max, tau_max} (:85-143).  Joint::getTransformation(q):
 * revolute R_pj (I + sin q K + (1 - cos q) K^2), t_pj; prismatic R_pj, t_pj + R_pj axis q (:38-47).
 * Chain link i (0 = base link): Link::getNominalParameters [m, m c, Ixx Ixy Ixz Iyy Iyz Izz about the link origin] (:399-417), mass,
 * centre of gravity in the link frame.  Any output may be NULL. */
int rdyn_chain_joint_constants(const rdyn_chain* chain, int i, double R_pj[9], double t_pj[3], double axis[3], double limits[5]);
int rdyn_chain_link_parameters(const rdyn_chain* chain, int i, double pi[10], double* mass, double cog[3]);
/* Chain::getNominalParameters primitives_impl.h:1382 -> pi[10 * joints_number] (HOST pointer) */
int rdyn_nominal_parameters(const rdyn_chain* chain, double* pi);
/* Rigid-body reduction of a chain whose input joints are a subset of its joints, listed in any order (fixed joints, primitives_impl.h:74-83,
 * or joints left out of setInputJointsName): links joined by non-input joints move as one body, so the ten regressor columns of a
 * link f + 1 hanging from a non-input joint are a CONSTANT linear image of the ten columns of the link the body's input joint
 * carries:  Y(:, 10 f + p) = sum_a Y(:, 10 body_joint[f] + a) X[f][a][p]   (zero for links upstream of the first input joint).
 * The regressor -> Gram / R-factor entry points use it internally (they sweep the reduced chain and expand the small result);
 * exposed for callers that reduce the parameter vector themselves.  Returns the number of bodies (= input joints; the bodies are
 * numbered in CHAIN order whatever the order of the input list), 0 when the chain has no reduction (every joint an input joint, or
 * more than RDYN_MAX_SWEPT_JOINTS input joints), < 0 on a null chain.
 * body_joint[n_joints]: chain index of the input joint whose child link is the body's reference frame, -1 = rides on the base;
 * X[n_joints][10][10] row-major (a, p); pi_body[10 * bodies]: the merged nominal parameters.  HOST pointers, each may be NULL. */
int rdyn_chain_reduction(const rdyn_chain* chain, int32_t* body_joint, double* X, double* pi_body);

/* ---- batched evaluation (device pointers) ------------------------------------------------------------ */
typedef enum rdyn_layout
{
  /* x[s][e] -- every sample's record is contiguous and is exactly the memory image of the Eigen object the
   * reference returns for that sample (VectorXd, column-major MatrixXd / Matrix6Xd, 3x4 column-major
   * Affine3d::affine()).  Drop-in layout.  Kinematic / torque / inertia outputs that start on a 128-byte line (any
   * hipMalloc does) are written in whole lines through wave-private LDS (rdyn_record_stage.h) at about the rate of the
   * element-major layout; other alignments are served correctly by 8-byte stores at 2-3x the time. */
  RDYN_LAYOUT_SAMPLE_MAJOR = 0,
  /* x[e][s] -- one N-vector per record element (structure of arrays).  Fully coalesced on the GPU;
   * for the regressor this IS a column-major (n*N) x P matrix whose row index is j*N + s. */
  RDYN_LAYOUT_ELEMENT_MAJOR = 1
} rdyn_layout;

typedef struct rdyn_batch
{
  int64_t n_samples;
  const double* q;    /* n_active values per sample                           */
  const double* dq;   /* may be NULL where the call does not need velocities  */
  const double* ddq;  /* may be NULL where the call does not need accelerations */
  int32_t layout;     /* rdyn_layout of q/dq/ddq AND of every output of the call (the regressor excepted, below) */
  int32_t device;     /* HIP device ordinal, -1 = current device */
  void* stream;       /* hipStream_t; NULL = the default stream */
} rdyn_batch;

/* Regressor element (sample s, active-joint row j, parameter column p) is written to
 *   Y[s * stride_sample + j * stride_row + p * stride_col]        (strides in doubles). */
typedef struct rdyn_regressor_layout
{
  int64_t stride_sample, stride_row, stride_col;
} rdyn_regressor_layout;
/* presets (n = active joints, P = 10 * joints_number, N = samples):
 *   per-sample Eigen image  getRegressor()[s] column-major n x P : {n*P, 1, n}
 *   stacked column-major (N*n) x P, row = s*n + j                : {n,   1, N*n}
 *   element-major = column-major (n*N) x P, row = j*N + s        : {1,   N, n*N}   <- fastest */

/* getTransformation primitives.h:452 -> T_bt[12] per sample: column-major 3x4 [R | p] (= Affine3d::affine()).
 * T_links (optional, may be NULL): getTransformations primitives.h:454 -> links_number x 12 per sample. */
int rdyn_transformation(const rdyn_chain* chain, const rdyn_batch* batch, double* T_bt, double* T_links);
/* getJacobian primitives.h:455 -> 6 x n column-major per sample */
int rdyn_jacobian(const rdyn_chain* chain, const rdyn_batch* batch, double* J);
/* getJacobianLink primitives.h:456 / primitives_impl.h:951-979 -> 6 x n column-major per sample, referred to the origin
 * of chain link `link_index` (0 = base .. joints_number = tool; names via rdyn_chain_link_name).  As in the
 * reference only the first `up` input columns are filled (up = input joints upstream of the link, :965-972), the rest
 * are zero; with the default chain-ordered input list those are exactly the link's parent joints.  (The by-name getters getTransformationLink / getTwistLink are the record
 * `link_index` of rdyn_transformation's T_links / rdyn_twist's twists.)  Stateless: evaluated at the given q, whereas
 * the reference's getJacobianLink ignores its q and uses the frames of the previous call (primitives_impl.h:953). */
int rdyn_jacobian_link(const rdyn_chain* chain, const rdyn_batch* batch, int link_index, double* J);
/* getTwist primitives.h:457 (needs q, dq) -> links_number x 6 per sample, [lin; ang] per link.
 * getDTwist primitives.h:463 (needs q, dq, ddq) -> same shape; either output may be NULL. */
int rdyn_twist(const rdyn_chain* chain, const rdyn_batch* batch, double* twists, double* dtwists);
/* getDTwistLinearPart (needs q, ddq) primitives.h:468, getDTwistNonLinearPart (q, dq) :473, getDDTwist (q, dq, ddq, dddq)
 * :488 -> links_number x 6 per sample each; any output may be NULL; dddq (layout of q) only for ddtwists. */
int rdyn_twist_parts(const rdyn_chain* chain, const rdyn_batch* batch, const double* dddq, double* dtwists_linear,
                     double* dtwists_nonlinear, double* ddtwists);
/* getDDTwistLinearPart (needs q, dddq) primitives.h:476 / primitives_impl.h:1126-1154 and getDDTwistNonLinearPart
 * (q, dq, ddq) primitives.h:480 / primitives_impl.h:1156-1183 -> links_number x 6 per sample each; either may be NULL. */
int rdyn_jerk_parts(const rdyn_chain* chain, const rdyn_batch* batch, const double* dddq, double* ddtwists_linear,
                    double* ddtwists_nonlinear);
/* getWrench(q, Dq, DDq, ext_wrenches_in_link_frame) primitives.h:530 / primitives_impl.h:1225-1262 -> links_number x 6 per
 * sample: the wrench transmitted through every link ([force; torque], base-frame coordinates, referred to the link's
 * origin); getWrenchTool is the last record.  ext_wrenches as in rdyn_joint_torque_ext, NULL = none. */
int rdyn_wrench(const rdyn_chain* chain, const rdyn_batch* batch, const double* ext_wrenches, double* wrenches);
/* getJointTorque(q, Dq, DDq) primitives.h:540 -> n per sample */
int rdyn_joint_torque(const rdyn_chain* chain, const rdyn_batch* batch, double* tau);
/* getJointTorque(q, Dq, DDq, ext_wrenches_in_link_frame) primitives.h:539: ext_wrenches = links_number x 6 per sample
 * ([force; torque] applied TO each link, in the link's frame; record layout = batch->layout).  The reference's
 * twist-form transform of the wrench (primitives_impl.h:1255) is reproduced as it is. */
int rdyn_joint_torque_ext(const rdyn_chain* chain, const rdyn_batch* batch, const double* ext_wrenches, double* tau);
/* getJointTorqueNonLinearPart(q, Dq) primitives.h:541 (DDq = 0; batch->ddq ignored) */
int rdyn_joint_torque_nonlinear(const rdyn_chain* chain, const rdyn_batch* batch, double* tau);
/* getRegressor primitives.h:543 fused with getJointTorque: writes Y (dense, structural zeros included) and,
 * if tau != NULL, tau = Y * nominal parameters (== getJointTorque, identity verified to 1e-13). */
int rdyn_regressor(const rdyn_chain* chain, const rdyn_batch* batch, double* tau, double* Y, const rdyn_regressor_layout* y_layout);
/* getJointInertia primitives.h:547 -> n x n column-major per sample */
int rdyn_joint_inertia(const rdyn_chain* chain, const rdyn_batch* batch, double* M);

/* Forward dynamics (no reference counterpart; defined by the two reference quantities it is built from): per sample ddq solves
 *     M ddq = tau - h
 * with M exactly what rdyn_joint_inertia returns for this chain AS CONFIGURED (input-joint selection and order included: joints that
 * are not input joints stay locked at 0) and h what rdyn_joint_torque_nonlinear returns (Coriolis, centrifugal and gravity terms).
 * batch->q, batch->dq required, batch->ddq ignored.  tau: n per sample, layout of batch->q; ddq: same shape and layout, may alias tau.
 * External wrenches and component (friction / spring) torques are additive in tau and are NOT parameters of this call:
 * rdyn_forward_dynamics_components takes the components and rdyn_forward_dynamics_ext both (below, behind the component types); they
 * subtract  tau_add of rdyn_components_regressor(..., tau_add)  and
 * rdyn_joint_torque_ext(q, 0, 0, ext) - rdyn_joint_torque(q, 0, 0)  inside the one launch.
 * status (device int32 per sample, may be NULL): 1 solved; -1 = M not positive definite by the rule of rdyn_local_ik (a Cholesky pivot
 * <= 1e-10 trace(M)): what a fixed joint listed as an input joint, or a tail of links without <inertial>, produces.  A -1 sample gets
 * quiet NaN in all its ddq entries; no sample's failure affects another sample.
 * Chains swept in registers (at most RDYN_MAX_SWEPT_JOINTS input joints; longer chains through their rigid-body reduction): one kernel
 * launch -- forward sweep, composite-rigid-body M and h, Cholesky and both triangular solves in registers; the workspace query returns
 * 0 and workspace may be NULL.  More input joints (up to RDYN_MAX_JOINTS, any order): element-major chunk images [M | h] of
 * chunk_samples samples in the workspace, factorised and solved in place (chunk_samples = 0: as many as keep an image within 128 MiB,
 * at least 16 384; results do not depend on the chunk size).  No allocation and no synchronisation: capturable into a graph once the
 * chain has been used on the device (first call outside capture, as for the other entry points). */
size_t rdyn_forward_dynamics_workspace_bytes(const rdyn_chain* chain, int64_t chunk_samples);
int rdyn_forward_dynamics(const rdyn_chain* chain, const rdyn_batch* batch, const double* tau, double* ddq, int32_t* status,
                          int64_t chunk_samples, void* workspace, size_t workspace_bytes);

/* Rollouts (no reference counterpart: the reference has no integrator): per sample, n_steps steps of size dt of
 *     x' = f(x),  x = (q, Dq),  f(x) = (Dq, FD(q, Dq, tau_t))
 * from the initial state batch->q, batch->dq (batch->ddq is ignored).  FD is exactly what rdyn_forward_dynamics defines for this chain AS
 * CONFIGURED (input-joint selection and order, joints that are not input joints locked at 0, the reduced companion of a long chain with at
 * most RDYN_MAX_SWEPT_JOINTS input joints, gravity).  The torques are held over a step (zero-order hold): step t uses the n values per
 * sample at tau + t * tau_step_stride, addressed like batch->q; tau_step_stride = 0 applies the same torques at every step.
 *   RDYN_INTEGRATOR_SEMI_IMPLICIT_EULER   DDq = FD(q_t, Dq_t, tau_t);  Dq_{t+1} = Dq_t + dt DDq;  q_{t+1} = q_t + dt Dq_{t+1}
 *   RDYN_INTEGRATOR_RK4                   the classical four-stage scheme (stage states x, x + dt/2 k1, x + dt/2 k2, x + dt k3; weights
 *                                         1/6, 1/3, 1/3, 1/6): four evaluations of FD per step, all with tau_t
 * dt is finite and not 0; a negative dt integrates backwards.
 * Outputs, each in the layout of batch->q and each optional (not all four NULL when n_samples > 0): q_end, dq_end = the state after
 * n_steps steps (q_end may alias batch->q and dq_end batch->dq); q_traj, dq_traj = a decimated trajectory: record k, at
 * + k * traj_step_stride doubles, is the state after step (k + 1) * traj_every; floor(n_steps / traj_every) records are written, so
 * traj_step_stride >= n * n_samples and traj_every >= 1 are required when either pointer is given.  n_steps = 0 copies the initial
 * state to the end state.
 * status (device int32 per sample, may be NULL): 1 if every evaluation of the sample solved, -1 if one did not by the pivot rule of
 * rdyn_forward_dynamics.  From the failing step on every state of that sample -- the end state and all later trajectory records -- is
 * quiet NaN; the failure is sticky and no sample affects another.
 * Friction and spring components depend on the state, so unlike in rdyn_forward_dynamics a caller cannot fold them into tau across
 * steps: rdyn_rollout_components (below, behind the component types) takes them.  External link wrenches give a joint torque that
 * depends on q and cannot be folded in either: rdyn_rollout_ext (below, behind rdyn_rollout_components) takes them and evaluates them
 * at every integrator stage.  No joint limits, no adaptive steps.
 * Chains swept in registers (at most RDYN_MAX_SWEPT_JOINTS input joints; longer chains through their rigid-body reduction): ONE kernel
 * launch for the whole horizon, the state in registers between the steps; a step reads n torques per sample and writes only the
 * trajectory record that is due; the workspace query returns 0 and workspace may be NULL.  More input joints (up to RDYN_MAX_JOINTS, any
 * order): the chunked route of rdyn_forward_dynamics once per stage on the batch's stream plus one element-wise update launch; state and
 * stage buffers live in the workspace behind the forward-dynamics images (chunk_samples as in rdyn_forward_dynamics; results do not
 * depend on it).  A horizon split anywhere into chained calls gives bitwise the state of the single call.
 * Errors, all RDYN_ERR_INVALID_ARGUMENT before any device work: NULL desc; NULL tau with n_steps > 0; all four outputs NULL with
 * n_samples > 0; n_steps < 0; dt zero or not finite; an unknown integrator; a trajectory pointer with traj_every < 1 or
 * traj_step_stride < n * n_samples; negative chunk_samples; a workspace smaller than the query's answer.  n_samples = 0 is RDYN_OK.
 * No allocation and no synchronisation: capturable into a graph once the chain has been used on the device. */
typedef enum rdyn_integrator { RDYN_INTEGRATOR_SEMI_IMPLICIT_EULER = 0, RDYN_INTEGRATOR_RK4 = 1 } rdyn_integrator;
typedef struct rdyn_rollout_desc
{
  int32_t n_steps;           /* T >= 0 */
  int32_t integrator;        /* rdyn_integrator */
  double dt;                 /* finite, != 0 */
  const double* tau;         /* step t at tau + t * tau_step_stride, addressed like batch->q */
  int64_t tau_step_stride;   /* in doubles; 0 = the same torques at every step */
  double* q_end;             /* state after T steps, layout of batch->q; may alias batch->q / batch->dq; each may be NULL */
  double* dq_end;
  double* q_traj;            /* optional: record k = the state after step (k + 1) * traj_every, at + k * traj_step_stride */
  double* dq_traj;
  int64_t traj_step_stride;  /* in doubles, >= n * N when a trajectory is requested */
  int32_t traj_every;        /* >= 1 when a trajectory is requested; floor(T / traj_every) records are written */
  int32_t* status;           /* per sample, may be NULL */
} rdyn_rollout_desc;
size_t rdyn_rollout_workspace_bytes(const rdyn_chain* chain, const rdyn_rollout_desc* desc, int64_t n_samples, int64_t chunk_samples);
int rdyn_rollout(const rdyn_chain* chain, const rdyn_batch* batch, const rdyn_rollout_desc* desc, int64_t chunk_samples, void* workspace,
                 size_t workspace_bytes);

/* Derivatives of the inverse dynamics (no reference counterpart).  With tau(q, Dq, DDq) exactly the function rdyn_joint_torque
 * evaluates for this chain AS CONFIGURED (input-joint selection and order, joints that are not input joints locked at 0, fixed joints,
 * gravity), per sample
 *     dtau_dq[i][k] = d tau_i / d q_k,   dtau_dv[i][k] = d tau_i / d Dq_k,   M[i][k] = d tau_i / d DDq_k (= rdyn_joint_inertia).
 * Each output: n x n column-major per sample in RDYN_LAYOUT_SAMPLE_MAJOR, x[e][s] with e = i + n k in RDYN_LAYOUT_ELEMENT_MAJOR (the
 * shape rules of rdyn_joint_inertia); rows and columns in input-joint order.  batch->q, dq and ddq are required.  Any output may be
 * NULL and is then not computed; all three NULL with n_samples > 0 is RDYN_ERR_INVALID_ARGUMENT.
 * External wrenches and component (friction / spring) torques are NOT parameters: both are additive in tau, so their derivatives are
 * the caller's to add -- in particular the Dq-derivative of a friction component (diagonal) goes on dtau_dv.
 * Derivatives of the forward dynamics DDq = FD(q, Dq, tau), with or without components, are rdyn_forward_dynamics_derivatives (below,
 * behind the component types): this call's matrices at DDq = FD(q, Dq, tau) with -M^-1 applied, in one launch.
 * Up to RDYN_MAX_SWEPT_JOINTS input joints (longer chains through their rigid-body reduction): one launch, a forward-mode tangent of
 * the recursive Newton-Euler sweep per input joint, O(n^2) per sample.  More input joints (up to RDYN_MAX_JOINTS, any order): one
 * launch with the per-joint state in LDS for the two derivative matrices, plus the launch of the inertia kernel when M is requested (two
 * launches then); RDYN_ERR_UNSUPPORTED if that state does not fit the LDS the device grants one workgroup (160 KB on gfx950, where
 * every chain up to RDYN_MAX_JOINTS fits; the figure is the runtime's, asked once per device).  No workspace, no allocation, no synchronisation: capturable into a graph once the chain
 * has been used on the device. */
int rdyn_joint_torque_derivatives(const rdyn_chain* chain, const rdyn_batch* batch, double* dtau_dq, double* dtau_dv, double* M);

/* Every getter of a sample in ONE call (no reference counterpart: the reference caches what a call computed on the way, m_last_q,
 * primitives_impl.h:886, 985, 1088, so its harness rosdyn_speed_test.cpp:109-185 pays for the frames once per sample).  Outputs as the
 * single-purpose entry points write them, record layout = batch->layout; any of them may be NULL:
 *   T_links (links x 12), J (6 x n), twists, dtwists (links x 6), tau, tau_nonlinear (n), M (n x n), Y with y_layout (NULL layout: the
 *   per-sample Eigen image {n P, 1, n}).  Needs q, dq, ddq.
 * Chains of <= RDYN_MAX_SWEPT_JOINTS joints: ONE kernel launch, the seven sweeps side by side (made for small batches: a sample per call
 * costs a launch, not seven -- the C++ facade's evaluateAll reads q / Dq / DDq from and writes the record to pinned host memory, so a
 * sample costs that launch and a synchronisation); longer chains: the same results by the single-purpose launches on the stream. */
typedef struct rdyn_all_outputs
{
  double* T_links;
  double* J;
  double* twists;
  double* dtwists;
  double* tau;
  double* tau_nonlinear;
  double* M;
  double* Y;
  const rdyn_regressor_layout* y_layout;
} rdyn_all_outputs;
int rdyn_evaluate_all(const rdyn_chain* chain, const rdyn_batch* batch, const rdyn_all_outputs* out);

/* ---- batched local inverse kinematics.
 * computeLocalIk primitives.h:510 / primitives_impl.h:1398-1433 (weight == NULL) and computeWeigthedLocalIk
 * primitives.h:526 / primitives_impl.h:1436-1468 (weight = 6 HOST doubles), one pose per batch entry:
 *   repeat: e = getFrameDistance(T_target, getTransformation(sol)) (frame_distance.h:44-49); if |weight o e| < toll -> converged;
 *           dq = argmin 1/2 dq'(J'WJ)dq - (J'We)'dq  s.t.  q_min <= sol + dq <= q_max  (Eigen::solve_quadprog);  sol += dq.
 * batch->q = the seeds (n_active per pose, batch->layout); T_target = 12 per pose, the column-major 3x4 [R|p] record
 * rdyn_transformation writes, same layout; sol = like the seeds (may alias them).  The reference bounds the loop by
 * wall-clock time (max_time, default 5 ms); here by max_iterations QP updates.  Per-pose results (device int32, either
 * may be NULL): status 1 = converged (the reference's `true`), 0 = not within max_iterations (`false`), -1 = J'WJ not
 * positive definite (a Cholesky pivot <= 1e-10 trace: more than 6 input joints or a singular pose; the reference's
 * Cholesky-based QP is undefined there),
 * -2 = bounds infeasible (q_min > q_max), -3 = QP iteration guard; iterations = QP updates performed.  On a failure
 * sol holds the last iterate. */
int rdyn_local_ik(const rdyn_chain* chain, const rdyn_batch* batch, const double* T_target, const double* weight, double toll,
                  int max_iterations, double* sol, int32_t* status, int32_t* iterations);
/* The pose-error functions of frame_distance.h on n_pairs pairs of frames (12 doubles each: the column-major 3x4 [R|p]
 * record of rdyn_transformation; `layout` as in rdyn_batch) -> 6 per pair [translation; rotation], expressed in frame w:
 *   RDYN_FRAME_DISTANCE_AXIS_ANGLE  getFrameDistance        frame_distance.h:44-49    [p_a - p_b; -R_wa (angle axis)(R_wa' R_wb)]
 *   RDYN_FRAME_DISTANCE_QUAT        getFrameDistanceQuat    frame_distance.h:73-86    [p_a - p_b; -2 R_wa imag(q_ab)], q_ab.w >= 0
 *   RDYN_FRAME_DISTANCE_QUAT_JAC    getFrameDistanceQuatJac frame_distance.h:112-126  [p_b - p_a; -2 R_wa imag(q_ab)] (the
 *       translation is measured the other way round there) and, if jacobian != NULL, the 6 x 6 column-major
 *       [I 0; 0 R_wa (w I - skew(imag q_ab)) R_wa'] per pair. */
typedef enum rdyn_frame_distance_kind
{
  RDYN_FRAME_DISTANCE_AXIS_ANGLE = 0,
  RDYN_FRAME_DISTANCE_QUAT = 1,
  RDYN_FRAME_DISTANCE_QUAT_JAC = 2
} rdyn_frame_distance_kind;
int rdyn_frame_distance(int64_t n_pairs, const double* T_wa, const double* T_wb, int layout, int kind, double* distance,
                        double* jacobian, int device, void* stream);
/* The same iteration with a Levenberg term: damping^2 is added to the diagonal of J'WJ before the QP (damping = 0 is
 * rdyn_local_ik).  No counterpart in the reference; it is what makes the loop usable where the reference's QP is singular
 * (7-DOF arms: J'J is 7 x 7 of rank 6) and near singular poses.
 * Chains of more than RDYN_MAX_SWEPT_JOINTS input joints (up to RDYN_MAX_JOINTS, any order; rdyn_long_ik.hip) solve the same
 * QP through a 6 x 6 system per working set.  There the pivot rule reads damping^2 <= 1e-10 trace(J'WJ + damping^2 I) -> -1:
 * with damping = 0 every pose that is not converged at its seed gets status -1 with 0 updates; a negative weight entry gives
 * -1 for every such pose too (J'WJ indefinite).  Fixed joints listed as inputs leave 6 or fewer moving joints possible on this
 * route: an update with fewer than six free moving joints (not held at a bound) whose damping^2 is at most 1e-10 trace of the 6 x 6
 * system is -1 as well (rdyn_local_ik solves that undamped case).  The statuses and `iterations` are those above. */
int rdyn_local_ik_damped(const rdyn_chain* chain, const rdyn_batch* batch, const double* T_target, const double* weight, double toll,
                         double damping, int max_iterations, double* sol, int32_t* status, int32_t* iterations);

/* ---- per-joint additive components: the extra regressor columns the identification step stacks next to
 * getRegressor.  Reference: FirstOrderPolynomialFriction friction_polynomial1.h:45-52
 * (columns [sign, omega]), SecondOrderPolynomialFriction friction_polynomial2.h:42-58 ([sign, omega, omega^2 sign]),
 * IdealSpring ideal_spring.h:64-70 ([q, 1]); getTorque = regressor row * parameters.  `joint` is the index of the
 * component's joint among the chain's ACTIVE joints (m_component_joint_number, base_component.h).
 * Constants follow friction_polynomial1.h:72-86: min_velocity < 1e-6 -> 1e-6, max_velocity <= 0 -> 1e6. */
typedef enum rdyn_component_type { RDYN_COMP_FRICTION1 = 0, RDYN_COMP_FRICTION2 = 1, RDYN_COMP_SPRING = 2 } rdyn_component_type;
typedef struct rdyn_component
{
  int32_t type;           /* rdyn_component_type */
  int32_t joint;          /* active-joint index */
  double min_velocity;    /* friction/constants/min_velocity */
  double max_velocity;    /* friction/constants/max_velocity */
  double parameters[3];   /* nominal: {coloumb, viscous} | {coloumb, first_order_viscous, second_order_viscous} | {elasticity, offset_effort} */
} rdyn_component;
/* Number of regressor columns of a component list (2, 3, 2 per type). */
int rdyn_components_columns(const rdyn_component* comps, int n_comps);
/* C(s, j, k) -> C[s*stride_sample + j*stride_row + k*stride_col] for k < rdyn_components_columns (dense: zero outside a
 * component's own joint row); pass Y + P*stride_col with Y's layout to append the columns to the inertial regressor.
 * tau_add (optional, layout of batch->q): += component torques.  C or tau_add may be NULL.  At most 30 components. */
int rdyn_components_regressor(const rdyn_component* comps, int n_comps, int n_active, const rdyn_batch* batch, double* C,
                              const rdyn_regressor_layout* c_layout, double* tau_add);

/* Forward dynamics and rollouts with components: the model rdyn_identification_gram / rdyn_identification_tsqr identify, simulated.
 * Let tau_c(q, Dq) be the component torque of the list: for active joint j the sum, over the components whose `joint` is j in list
 * order, of row . parameters -- exactly what rdyn_components_regressor accumulates into a zero-initialised tau_add (the same
 * saturations, the same min_velocity / max_velocity constants, the same fma order).  Then
 *     FD_c(q, Dq, tau) = FD(q, Dq, tau - tau_c(q, Dq))
 * with FD the function of rdyn_forward_dynamics for the chain AS CONFIGURED (input-joint selection and order, locked joints, the
 * reduced companion of a long chain with at most RDYN_MAX_SWEPT_JOINTS input joints, the chunked route with more).  component.joint
 * indexes the active joints in INPUT order, whatever order the chain's joints are swept in.
 *   rdyn_forward_dynamics_components   ddq = FD_c(q, Dq, tau); every other argument, the status, the aliasing rule (ddq may alias tau)
 *                                      and the workspace are those of rdyn_forward_dynamics.
 *   rdyn_rollout_components            integrates x' = (Dq, FD_c(q, Dq, tau_t)); tau_c is evaluated at EVERY integrator stage at that
 *                                      stage's own state: RK4 at (stage state, stage velocity), semi-implicit Euler at (q_t, Dq_t).
 *                                      Everything else is rdyn_rollout's: the descriptor, status and sticky NaN, aliasing, trajectory
 *                                      records, the bitwise split of the horizon, independence from the chunk size.
 * n_comps = 0 is allowed (comps may then be NULL) and IS rdyn_forward_dynamics / rdyn_rollout: the same kernels, the same bits.
 * n_comps > 0: a NULL list, more than 30 components, an unknown type or a joint outside [0, n_active) are RDYN_ERR_INVALID_ARGUMENT
 * before any device work, as are all argument errors of the two base calls.  The workspace queries of the base calls answer for these
 * calls too (no extra workspace).  Chains swept in registers: still ONE launch, the list in the kernel arguments; more input joints: the
 * solve kernel of the chunked route reads the sample's q and Dq where it reads tau.  No allocation, no synchronisation, capturable into
 * a graph as the base calls are.
 * Chatter: the friction "sign" is linear inside +-min_velocity with slope coulomb / min_velocity -- continuous and bounded, but stiff.
 * When dt * coulomb / (min_velocity * M_jj) is not small, an explicit integrator chatters inside that band; the amplitude stays
 * bounded by dt * coulomb / M_jj.  There is no implicit integrator. */
int rdyn_forward_dynamics_components(const rdyn_chain* chain, const rdyn_batch* batch, const rdyn_component* comps, int n_comps,
                                     const double* tau, double* ddq, int32_t* status, int64_t chunk_samples, void* workspace,
                                     size_t workspace_bytes);
int rdyn_rollout_components(const rdyn_chain* chain, const rdyn_batch* batch, const rdyn_rollout_desc* desc, const rdyn_component* comps,
                            int n_comps, int64_t chunk_samples, void* workspace, size_t workspace_bytes);

/* Forward dynamics and rollouts with external link wrenches: the forward side of rdyn_joint_torque_ext / getJointTorque(q, Dq, DDq,
 * ext_wrenches_in_link_frame).  Let tau_E(q, ext) be the joint torque of the wrenches alone,
 *     tau_E = rdyn_joint_torque_ext(q, 0, 0, ext) - rdyn_joint_torque(q, 0, 0)
 * (equivalently rdyn_joint_torque_ext(q, 0, 0, ext) of the same chain with zero gravity): a wrench [force; torque] applied TO a chain
 * link, given in that link's own frame, with the reference's twist-form transform (primitives_impl.h:1255) reproduced as it is.  tau_E is
 * linear in ext, depends on q and not on Dq, and the base link's record does not enter.  Then
 *     FD_E(q, Dq, tau, ext) = FD_c(q, Dq, tau - tau_E(q, ext))
 * with FD_c the function of rdyn_forward_dynamics_components for the chain AS CONFIGURED (input-joint selection and order, locked joints,
 * gravity, the component list; n_comps = 0 is the plain call).
 *   rdyn_forward_dynamics_ext   ddq = FD_E(q, Dq, tau, ext); every other argument, the status and the aliasing rule (ddq may alias tau)
 *                               are those of rdyn_forward_dynamics.  ext->step_stride is not read.
 *   rdyn_rollout_ext            integrates x' = (Dq, FD_E(q, Dq, tau_t, ext_t)); the wrench of step t is held over the step like tau_t
 *                               and evaluated at EVERY integrator stage at that stage's own q.  Everything else is rdyn_rollout's: the
 *                               descriptor, sticky status, aliasing, trajectory records, the bitwise split of the horizon (with a
 *                               per-step wrench sequence too: the later call starts at w + t0 * step_stride), independence from the
 *                               chunk size.
 * ext: see rdyn_ext_wrenches.  link = -1: w holds links_number x 6 doubles per sample, exactly the argument of rdyn_joint_torque_ext
 * (sample-major: record after record; element-major: element e of sample s at w[e * n_samples + s]); link >= 0: 6 doubles per sample,
 * the wrench of that one chain link (0 = the base link, which changes nothing; joints_number = the tool), the others zero.  The wrench
 * arrays must not overlap an output.
 * ext == NULL or ext->w == NULL IS rdyn_forward_dynamics_components / rdyn_rollout_components: the same kernels, the same bits, and the
 * workspace queries equal the base queries.
 * Status: the pivot rule of rdyn_forward_dynamics looks at M, which the wrenches do not enter.  A non-finite wrench entry therefore makes
 * the sample's ddq NaN by propagation with status 1 in rdyn_forward_dynamics_ext; in a rollout the NaN state fails the pivot rule at the
 * next evaluation, so the sample's status is -1 (and its state quiet NaN from then on) unless the entry was first read in the last
 * evaluation of the horizon, where the end state is NaN with status 1.
 * Chains of at most RDYN_MAX_SWEPT_JOINTS chain joints: still ONE launch, for one evaluation and for a whole horizon; the wrench enters
 * the link's net wrench inside the forward sweep, no workspace.  More than RDYN_MAX_SWEPT_JOINTS input joints: the chunked route, whose
 * wrench recursion takes the wrenches as it writes h (CORRECT, NOT FAST); the workspace is the base call's.  Long chains served through a
 * reduced companion (more than RDYN_MAX_SWEPT_JOINTS chain joints, at most that many input joints): the wrenches belong to the original
 * links, which the companion no longer has, so WITH wrenches these chains take the chunked route on the original chain (workspace: ask
 * the queries below with the ext you will pass); without wrenches nothing changes for them.
 * Errors, all RDYN_ERR_INVALID_ARGUMENT before any device work: every argument error of the base calls, and with wrenches a link outside
 * [-1, joints_number], in rollouts a negative step_stride or a non-zero one smaller than one step's record (6 * links_number * n_samples,
 * or 6 * n_samples for one link).  n_samples = 0 is RDYN_OK.  No allocation and no synchronisation: capturable into a graph once the
 * chain has been used on the device. */
typedef struct rdyn_ext_wrenches
{
  const double* w;      /* link = -1: links_number x 6 per sample, exactly the argument of rdyn_joint_torque_ext (record layout =
                           batch->layout); link >= 0: 6 doubles per sample, [force; torque] applied to that chain link in its frame */
  int32_t link;         /* -1 = every link; else a chain link index 0 .. joints_number (the tool is joints_number) */
  int64_t step_stride;  /* rollouts only, in doubles: step t at w + t * step_stride; 0 = the same wrenches at every step */
} rdyn_ext_wrenches;
size_t rdyn_forward_dynamics_ext_workspace_bytes(const rdyn_chain* chain, const rdyn_ext_wrenches* ext, int64_t chunk_samples);
int rdyn_forward_dynamics_ext(const rdyn_chain* chain, const rdyn_batch* batch, const rdyn_component* comps, int n_comps,
                              const rdyn_ext_wrenches* ext, const double* tau, double* ddq, int32_t* status, int64_t chunk_samples,
                              void* workspace, size_t workspace_bytes);
size_t rdyn_rollout_ext_workspace_bytes(const rdyn_chain* chain, const rdyn_rollout_desc* desc, const rdyn_ext_wrenches* ext,
                                        int64_t n_samples, int64_t chunk_samples);
int rdyn_rollout_ext(const rdyn_chain* chain, const rdyn_batch* batch, const rdyn_rollout_desc* desc, const rdyn_component* comps,
                     int n_comps, const rdyn_ext_wrenches* ext, int64_t chunk_samples, void* workspace, size_t workspace_bytes);

/* Closed-loop rollouts (no reference counterpart): rdyn_rollout_ext with a joint-space PD controller and actuator limits in the loop
 * (the model-based laws -- gravity compensation, computed torque -- are rdyn_rollout_model_feedback's, below).  A
 * feedback torque depends on the state, so like the components it cannot be folded into tau across steps.  n = the number of active
 * joints; every array of rdyn_feedback is in INPUT order.  At an evaluation with state (q, Dq) in step t, per sample and joint j,
 *     u_j = fma(kd_j, Dq_ref[t]_j - Dq_j, fma(kp_j, q_ref[t]_j - q_j, tau_ff[t]_j))        (this order, on every route)
 *     u_j = u_j > lim_j ? lim_j : (u_j < -lim_j ? -lim_j : u_j)                             (only with tau_limit)
 *     DDq = FD_E(q, Dq, u, ext_t)
 * tau_ff is the descriptor's tau sequence, unchanged in meaning: it is now the feed-forward term.  FD_E is the function of
 * rdyn_rollout_ext: the clamp acts on the actuator command alone, component and wrench torques are applied behind it as before.  The
 * clamp is two comparisons, so a NaN command stays NaN.  kd == NULL: the velocity term is not formed and dq_ref is not read; dq_ref ==
 * NULL with kd: Dq_ref = 0.
 *   hold = 1   the digital controller: the command is formed once per step from the state at the start of the step and held over all
 *              stages of the step, exactly as tau_t is held.
 *   hold = 0   the continuous law: the command is formed anew at every integrator stage at that stage's own (q, Dq), as the components
 *              are (RK4: the stage state and the stage velocity).
 * Semi-implicit Euler has one evaluation per step, at the start state: the two modes are the same computation and give the same bits.
 * References: step t at q_ref + t * ref_step_stride (and dq_ref likewise), addressed like batch->q; ref_step_stride = 0 is a constant
 * set point.  Gains: gains_per_sample = 0: kp, kd hold n values shared by all samples; 1: addressed like batch->q.  tau_limit: n values,
 * shared; positive values are the caller's business.
 * tau_traj (optional output, layout of batch->q): record k, at + k * desc->traj_step_stride, holds the command u of the FIRST evaluation of
 * step (k + 1) * traj_every - 1 -- the step whose end state is state record k; under hold = 1 that is the command of the whole step.  It
 * counts as an output for the "every output is null" rule and needs traj_every >= 1 and the stride condition of the state trajectories.
 * A sample whose status was already -1 when the step began gets quiet NaN; in the step at which a sample fails the record holds the
 * command that was applied (NaN by propagation where a NaN input caused the failure).
 * fb == NULL IS rdyn_rollout_ext: the same kernels, the same bits, the same workspace query.  ext == NULL (or ext->w == NULL) and
 * n_comps = 0 behave as in rdyn_rollout_ext.  Sticky status, aliasing of the end state, trajectory records and independence from the chunk
 * size are rdyn_rollout's.  A horizon split anywhere into chained calls gives the same bits: the later call starts its references at
 * + t0 * ref_step_stride, as it does for torques and wrenches.
 * Status: a non-finite entry of a reference, a gain or a limit follows the rule of non-finite wrenches (rdyn_rollout_ext): the command and
 * with it the state become NaN by propagation, the NaN state fails the pivot rule at the next evaluation, so the sample's status is -1 and
 * its state quiet NaN from then on (unless the entry was first read in the last evaluation of the horizon: NaN end state, status 1).
 * Neighbouring samples are untouched.
 * Chains swept in registers (rdyn_rollout's rule; with wrenches rdyn_rollout_ext's): still ONE launch for the horizon, no workspace.
 * The chunked route: one element-wise launch forms u before the pass of every evaluation whose command is formed anew (once per step
 * under hold = 1, once per stage under hold = 0) into one more state array of the workspace:
 *     rdyn_rollout_feedback_workspace_bytes = rdyn_rollout_ext_workspace_bytes + align256(n * n_samples * sizeof(double))
 * (align256 rounds up to a multiple of 256 bytes; 0 stays 0 where the ext query answers 0).
 * Errors, all RDYN_ERR_INVALID_ARGUMENT before any device work: every argument error of rdyn_rollout_ext; NULL q_ref or NULL kp; a
 * negative ref_step_stride or a non-zero one below n * n_samples; hold or gains_per_sample outside {0, 1}; tau_traj without traj_every >= 1
 * and traj_step_stride >= n * n_samples.  n_samples = 0 is RDYN_OK.  No allocation and no synchronisation: capturable into a graph once
 * the chain has been used on the device.
 * Reverse mode: rdyn_rollout_adjoint_feedback (below) is the transpose of this call, the law included, for the chains this call runs
 * in registers, and rosdyn_amd.autograd.rollout serves the closed loop through it.  On the chunked route it answers
 * RDYN_ERR_UNSUPPORTED: there rosdyn_amd.autograd does not serve the closed loop yet (the follow-up named at that call). */
typedef struct rdyn_feedback
{
  const double* q_ref;        /* step t at q_ref + t * ref_step_stride, addressed like batch->q; required */
  const double* dq_ref;       /* same addressing; NULL = zero */
  int64_t ref_step_stride;    /* doubles; 0 = a constant set point; otherwise >= n * n_samples */
  const double* kp;           /* required */
  const double* kd;           /* NULL = zero (dq_ref is then not read) */
  int32_t gains_per_sample;   /* 0: kp, kd hold n values in input order, shared by all samples; 1: addressed like batch->q */
  int32_t hold;               /* 1: the command of the step's start state serves the whole step; 0: formed at every stage */
  const double* tau_limit;    /* n values in input order; NULL = no limit */
  double* tau_traj;           /* optional output: the command records, see above */
} rdyn_feedback;
size_t rdyn_rollout_feedback_workspace_bytes(const rdyn_chain* chain, const rdyn_rollout_desc* desc, const rdyn_ext_wrenches* ext,
                                             const rdyn_feedback* fb, int64_t n_samples, int64_t chunk_samples);
int rdyn_rollout_feedback(const rdyn_chain* chain, const rdyn_batch* batch, const rdyn_rollout_desc* desc, const rdyn_component* comps,
                          int n_comps, const rdyn_ext_wrenches* ext, const rdyn_feedback* fb, int64_t chunk_samples, void* workspace,
                          size_t workspace_bytes);

/* Closed-loop rollouts under a model-based law (no reference counterpart): rdyn_rollout_feedback with the controller's own model of the
 * arm inside the loop -- PD with gravity compensation, and computed torque (inverse-dynamics control).  `model` is a chain of its own
 * (rdyn_chain_with_parameters makes "the same arm with other inertial parameters"; it may be the plant chain itself); its geometry,
 * gravity and parameters may differ from the plant's: the mismatch is what such a simulation is for.  fb is the rdyn_feedback of
 * rdyn_rollout_feedback: references, gains, hold, limits and tau_traj keep their addressing and meaning.
 * RNEA_m(q, v, a) = the function rdyn_joint_torque evaluates for `model` as configured (its own inertial parameters, geometry and
 * gravity; input order; locked joints at 0); no components and no wrenches enter the model.  At an evaluation at the state (q, Dq) in
 * step t, per sample and input joint j:
 *   RDYN_LAW_COMPUTED_TORQUE
 *     a_j = fma(kd_j, Dq_ref[t]_j - Dq_j, fma(kp_j, q_ref[t]_j - q_j, ddq_ref[t]_j))
 *     u   = tau_ff[t] + RNEA_m(q, Dq, a),  then the clamp of rdyn_rollout_feedback
 *     kp and kd are in 1/s^2 and 1/s here.  kd == NULL: the velocity term is not formed and dq_ref is not read.
 *   RDYN_LAW_GRAVITY_COMPENSATION
 *     u_j = the unclamped PD command of rdyn_rollout_feedback (the same fma order) + RNEA_m(q, 0, 0)_j,  then the clamp
 * hold decides where the law is formed, the model sweep included: hold = 1 at the head of the step, held over the stages; hold = 0 at
 * every stage at that stage's own state.  Semi-implicit Euler is one computation under both modes.  Components and wrenches of the
 * plant act behind the clamp, as in rdyn_rollout_feedback; tau_traj, the sticky status, NaN propagation, aliasing and the split horizon
 * (ddq_ref advances by t0 * ref_step_stride like the other references) are that call's.
 * Routing, before any device work:
 *   mfb == NULL IS rdyn_rollout_feedback: the same kernels, the same bits, the same workspace query.
 *   with mfb, the call serves the chains rdyn_rollout_feedback runs in registers: at most RDYN_MAX_SWEPT_JOINTS swept joints, longer
 *     chains through their reduced companion (the model's companion is swept for the law).  ONE launch for the horizon, the workspace
 *     query answers 0, no allocation and no synchronisation: capturable into a graph once both chains have been used on the device.
 *   chains for which rdyn_rollout_feedback takes the chunked route: RDYN_ERR_UNSUPPORTED (the message names the route); the query
 *     answers 0.
 * Errors, all RDYN_ERR_INVALID_ARGUMENT before any device work: every argument error of rdyn_rollout_feedback, fb being required once
 * mfb is given; a NULL model; an unknown law; ddq_ref with RDYN_LAW_GRAVITY_COMPENSATION; a model that differs from the chain in the
 * number of chain joints, in any joint type, in the input-joint selection or order, or in the swept joint count of the chain actually
 * swept.  n_samples = 0 is RDYN_OK.
 * Reverse mode is the follow-up: rdyn_rollout_adjoint_feedback is the transpose of the PD law alone and does not take a
 * rdyn_model_feedback; Chain.rolloutAdjoint and rosdyn_amd.autograd raise an error when handed a rosdyn_amd.ModelFeedback. */
typedef enum rdyn_feedback_law { RDYN_LAW_GRAVITY_COMPENSATION = 1, RDYN_LAW_COMPUTED_TORQUE = 2 } rdyn_feedback_law;
typedef struct rdyn_model_feedback
{
  const rdyn_chain* model;  /* the controller's model of the arm; may be the plant chain itself; required */
  int32_t law;              /* rdyn_feedback_law */
  const double* ddq_ref;    /* computed torque only: step t at ddq_ref + t * fb->ref_step_stride, addressed like batch->q; NULL = zero */
} rdyn_model_feedback;
size_t rdyn_rollout_model_feedback_workspace_bytes(const rdyn_chain* chain, const rdyn_rollout_desc* desc, const rdyn_ext_wrenches* ext,
                                                   const rdyn_feedback* fb, const rdyn_model_feedback* mfb, int64_t n_samples,
                                                   int64_t chunk_samples);
int rdyn_rollout_model_feedback(const rdyn_chain* chain, const rdyn_batch* batch, const rdyn_rollout_desc* desc, const rdyn_component* comps,
                                int n_comps, const rdyn_ext_wrenches* ext, const rdyn_feedback* fb, const rdyn_model_feedback* mfb,
                                int64_t chunk_samples, void* workspace, size_t workspace_bytes);

/* Derivatives of the forward dynamics (no reference counterpart): the linearisation of DDq = FD_c(q, Dq, tau).  Per sample, with FD_c the
 * function of rdyn_forward_dynamics_components for the chain AS CONFIGURED (input-joint selection and order, locked joints, the reduced
 * companion, gravity; n_comps = 0 is rdyn_forward_dynamics),
 *     ddq            = FD_c(q, Dq, tau)                                   required; layout of batch->q; may alias tau
 *     dddq_dq[i][k]  = d DDq_i / d q_k   = -M^-1 (dtau_dq + diag d tau_c / d q)
 *     dddq_dv[i][k]  = d DDq_i / d Dq_k  = -M^-1 (dtau_dv + diag d tau_c / d Dq)
 *     minv           = d DDq / d tau     = M^-1, both triangles (the same bits in both)
 * dtau_dq, dtau_dv the matrices of rdyn_joint_torque_derivatives evaluated at this sample's own ddq.  Each matrix has the record shape
 * and layouts of rdyn_joint_torque_derivatives (n x n column-major per sample in RDYN_LAYOUT_SAMPLE_MAJOR, x[e][s] with e = i + n k in
 * RDYN_LAYOUT_ELEMENT_MAJOR, rows and columns in input order), is optional and is not computed when NULL; all three NULL with
 * n_samples > 0 is RDYN_ERR_INVALID_ARGUMENT.  batch->q and dq are required, batch->ddq is ignored.
 * Component slopes, with the constants rdyn_components_regressor uses (min_velocity, max_velocity as sanitised there): a spring adds
 * parameters[0] to d tau_c / d q of its joint.  Friction at x = Dq_j, omega = clamp(x, +-max_velocity): omega' = 1 for |x| < max_velocity,
 * else 0; sg' = 1 / min_velocity for |omega| < min_velocity, else 0; RDYN_COMP_FRICTION1 adds omega' (p0 sg' + p1), RDYN_COMP_FRICTION2
 * omega' (p0 sg' + p1 + p2 (2 omega sg + omega^2 sg')) to d tau_c / d Dq.  Several components on one joint add in list order.  EXACTLY AT
 * A KINK (|x| = max_velocity, |omega| = min_velocity) the slope is the OUTER one-sided one: that of the saturated side.
 * status (may be NULL) is 1 or -1 by the pivot rule of rdyn_forward_dynamics; a -1 sample gets quiet NaN in ddq and in every matrix
 * requested; no sample affects another.
 * Up to RDYN_MAX_SWEPT_JOINTS input joints (longer chains through their rigid-body reduction): ONE launch, one lane per sample; nothing
 * touches device memory between the inputs and the outputs; the workspace query returns 0.  More input joints: per chunk the chunked
 * route of rdyn_forward_dynamics, the derivative kernel of rdyn_joint_torque_derivatives at that ddq into the caller's matrices, and one
 * launch that solves them in place; the workspace is the forward-dynamics image plus one status word per sample of a chunk
 * (chunk_samples as in rdyn_forward_dynamics; results do not depend on it); RDYN_ERR_UNSUPPORTED where rdyn_joint_torque_derivatives
 * answers so.
 * Errors, all RDYN_ERR_INVALID_ARGUMENT before any device work: every argument error of rdyn_forward_dynamics_components with the same
 * rules for the component list; NULL ddq or tau with samples; all matrices NULL; a workspace smaller than this call's own query.
 * n_samples = 0 is RDYN_OK.  No allocation, no synchronisation: capturable into a graph once the chain has been used on the device.
 * A semi-implicit-Euler rollout linearises in one call: feed the T N trajectory records of rdyn_rollout through it as one batch;
 * A_t, B_t are I + dt (...) of its outputs.  (A gradient through a rollout, either integrator, needs none of the matrices:
 * rdyn_rollout_adjoint below.) */
size_t rdyn_forward_dynamics_derivatives_workspace_bytes(const rdyn_chain* chain, int64_t chunk_samples);
int rdyn_forward_dynamics_derivatives(const rdyn_chain* chain, const rdyn_batch* batch, const rdyn_component* comps, int n_comps,
                                      const double* tau, double* ddq, double* dddq_dq, double* dddq_dv, double* minv, int32_t* status,
                                      int64_t chunk_samples, void* workspace, size_t workspace_bytes);

/* Reverse-mode product of the forward dynamics (no reference counterpart): what a gradient needs of the linearisation above, without the
 * matrices.  Per sample, with FD_c exactly the function of rdyn_forward_dynamics_components for the chain AS CONFIGURED and dddq_dq,
 * dddq_dv, M^-1 exactly the matrices rdyn_forward_dynamics_derivatives defines (component slopes and the outer-side rule at a kink
 * included), for a seed ddq_bar on DDq
 *     q_bar   = dddq_dq' ddq_bar        dq_bar  = dddq_dv' ddq_bar        tau_bar = M^-1 ddq_bar
 *     ddq     = FD_c(q, Dq, tau)        optional; the bits of rdyn_forward_dynamics_components
 * All vectors hold n doubles per sample in the layout of batch->q.  Each of q_bar, dq_bar, tau_bar is optional and is not computed when
 * NULL; all three NULL with n_samples > 0 is RDYN_ERR_INVALID_ARGUMENT.  tau_bar may alias ddq_bar.  batch->q and dq are required,
 * batch->ddq is ignored.
 * status (may be NULL) is 1 or -1 by the pivot rule of rdyn_forward_dynamics; a sample with a non-finite entry in q, Dq, tau or ddq_bar
 * is -1 too.  A -1 sample gets quiet NaN in every output requested; no sample affects another.
 * Up to RDYN_MAX_SWEPT_JOINTS input joints (longer chains through their rigid-body reduction): ONE launch, one lane per sample, ONE pair of
 * triangular solves per sample (w = M^-1 ddq_bar, with the factor still in registers) where the derivative call needs 3 n, and every
 * column of dtau / d(q, Dq) collapses into its dot product with w while its rows appear: 4 n doubles in, at most 4 n out, no n x n object
 * anywhere; the workspace query returns 0.  More input joints (up to RDYN_MAX_JOINTS, any order): CORRECT, NOT FAST -- per chunk the
 * chunked rdyn_forward_dynamics_derivatives into element-major matrices in the workspace and one launch that forms the three
 * transposed products; the workspace is that call's plus (3 n n + n) doubles per sample of a chunk (chunk_samples as in
 * rdyn_forward_dynamics; results do not depend on it); RDYN_ERR_UNSUPPORTED where rdyn_joint_torque_derivatives answers so.
 * Errors, all RDYN_ERR_INVALID_ARGUMENT before any device work: every argument error of rdyn_forward_dynamics_components with the same
 * rules for the component list (its ddq is optional here); NULL tau or ddq_bar with samples; all three products NULL; a negative
 * chunk_samples; a workspace smaller than this call's own query.  n_samples = 0 is RDYN_OK.  No allocation, no synchronisation:
 * capturable into a graph once the chain has been used on the device. */
size_t rdyn_forward_dynamics_vjp_workspace_bytes(const rdyn_chain* chain, int64_t chunk_samples);
int rdyn_forward_dynamics_vjp(const rdyn_chain* chain, const rdyn_batch* batch, const rdyn_component* comps, int n_comps, const double* tau,
                              const double* ddq_bar, double* q_bar, double* dq_bar, double* tau_bar, double* ddq, int32_t* status,
                              int64_t chunk_samples, void* workspace, size_t workspace_bytes);

/* Reverse-mode product of the forward dynamics with respect to the PARAMETERS of the model (no reference counterpart): the gradient
 * output-error identification needs.  Per sample FD_c, w = tau_bar = M^-1 ddq_bar, ddq and the status are exactly those of
 * rdyn_forward_dynamics_vjp (the same bits), and since tau = Y(q, Dq, DDq) pi + C(q, Dq) p at that ddq,
 *     pi_bar   = -Y(q, Dq, ddq)' w     P = 10 joints_number doubles, the order of rdyn_nominal_parameters / the columns of rdyn_regressor
 *     comp_bar = -C(q, Dq)' w          K = rdyn_components_columns doubles, the columns of rdyn_components_regressor (the saturated rows:
 *                                      the same constants, the same clamps)
 * Y and C are never formed: one more forward recursion over the links with the joint rates w, about 60 flops per link.
 *   pi_bar, comp_bar          the per-sample rows: P (K) doubles per sample, contiguous per sample in RDYN_LAYOUT_SAMPLE_MAJOR, x[col][s] in
 *                             RDYN_LAYOUT_ELEMENT_MAJOR (the batch's layout)
 *   pi_bar_sum, comp_bar_sum  P (K) doubles: the sums of the rows over the samples with status 1; accumulate = 0 overwrites, 1 adds to
 *                             what is there
 *   tau_bar, ddq, status      as in rdyn_forward_dynamics_vjp; tau_bar may alias ddq_bar
 * Every output may be NULL and is then not computed; pi_bar, comp_bar, both sums and tau_bar all NULL with n_samples > 0 is
 * RDYN_ERR_INVALID_ARGUMENT.  A status -1 sample gets quiet NaN in its rows (and in tau_bar, ddq) and adds nothing to the sums; no sample
 * affects another.
 * The sums are reproducible bit for bit from run to run for the same n_samples and layout: every wave adds its 64 samples in a fixed
 * butterfly, a second launch adds the waves' partials in a fixed order; no floating-point atomics.
 * Up to RDYN_MAX_SWEPT_JOINTS input joints: ONE launch, plus two small ones when a sum is asked for.  A longer chain with at most that
 * many input joints runs on its reduced companion; the rows and sums of its own links are X_f' (those of the body f rides on), X_f of
 * rdyn_chain_reduction, links upstream of the first input joint 0 -- on the device, no host round trip.  More input joints (up to
 * RDYN_MAX_JOINTS, any order): CORRECT, NOT FAST -- the chunked route of rdyn_forward_dynamics_vjp gives tau_bar, ddq and the status, then
 * per chunk an element-major image [Y | C] at that ddq (the writer of rdyn_identification_gram_wide) and one launch that forms the rows;
 * the sums are fixed-order column sums of the rows.  Neither rows nor sums depend on chunk_samples.
 * Workspace, from the query below.  Swept chains (needed only when a sum is asked for): (ceil(n_samples / 64) + 1) (10 n_swept + K)
 * doubles.  The chunked route (always needed): rdyn_forward_dynamics_vjp's, 2 n n_samples doubles and n_samples status words, the
 * image of one chunk (n (P + K + 1) doubles per sample of it) and (P + K) (n_samples + 1) doubles for the rows and the totals.
 * Errors, all RDYN_ERR_INVALID_ARGUMENT before any device work: those of rdyn_forward_dynamics_vjp; every product NULL; accumulate
 * other than 0 or 1; a workspace smaller than the query's answer when a sum is asked for.  n_samples = 0 is RDYN_OK.  No allocation, no
 * synchronisation: capturable into a graph once the chain has been used on the device. */
size_t rdyn_forward_dynamics_parameter_vjp_workspace_bytes(const rdyn_chain* chain, const rdyn_component* comps, int n_comps,
                                                           int64_t n_samples, int64_t chunk_samples);
int rdyn_forward_dynamics_parameter_vjp(const rdyn_chain* chain, const rdyn_batch* batch, const rdyn_component* comps, int n_comps,
                                        const double* tau, const double* ddq_bar, double* pi_bar, double* comp_bar, double* pi_bar_sum,
                                        double* comp_bar_sum, int accumulate, double* tau_bar, double* ddq, int32_t* status,
                                        int64_t chunk_samples, void* workspace, size_t workspace_bytes);

/* Adjoint of a rollout (no reference counterpart): the exact transpose of the discrete scheme rdyn_rollout / rdyn_rollout_components
 * implement, backwards over the whole horizon -- both integrators; the RK4 stage states are rebuilt inside.  (The forward-mode recipe at
 * the end of rdyn_forward_dynamics_derivatives' comment still holds for semi-implicit Euler; this call replaces it where a gradient,
 * not the matrices A_t, B_t, is wanted.)  With x_t = (q_t, Dq_t), x_0 = the batch's q, dq and T = n_steps:
 *     lambda_T = g_end + g_traj[T - 1]
 *     for t = T - 1 .. 0:   (lambda_t, gtau_t) = step'(x_t, tau_t; lambda_{t + 1});   for t >= 1: lambda_t += g_traj[t - 1]
 *     gq0, gdq0 = lambda_0
 * T = 1 reads no trajectory; T = 0 copies the end seeds to gq0, gdq0.  With vjp(q, v, tau; a_bar) -> (q_bar, v_bar, tau_bar) the product
 * of rdyn_forward_dynamics_vjp, the step transposes are, in this order,
 *   semi-implicit Euler (v' = v + dt a, q' = q + dt v'):   lv* = lv' + dt lq';   mu = dt lv*;   (q_bar, v_bar, tau_bar) = vjp(x_t, tau_t; mu);
 *       lq = lq' + q_bar;   lv = lv* + v_bar;   gtau_t = tau_bar
 *   RK4:   the stage states X1 .. X4 from x_t as the forward call builds them (three plain evaluations);   kq_i = dt b_i lq',
 *       kv_i = dt b_i lv' with b = 1/6, 1/3, 1/3, 1/6;   x_bar = lambda';   for i = 4, 3, 2, 1:   (q_bar, v_bar, tau_bar) = vjp(X_i, tau_t; kv_i),
 *       X_bar_i = (q_bar, kq_i + v_bar),   gtau_t += tau_bar,   x_bar += X_bar_i,   for i > 1: k_{i-1} += c_i X_bar_i with c = ., dt/2, dt/2, dt;
 *       lambda_t = x_bar.
 * Component torques and their slopes are taken at each stage's own state, as in the forward call.
 * status (may be NULL): -1 if any evaluation of the sample fails the pivot rule or meets a non-finite value; from that backward step on
 * every output of the sample is quiet NaN (gtau of the later steps, already written, stays).  A sample whose forward rollout reported
 * -1 has NaN records and is NaN in every gradient output.
 * Split horizons: with gtau_step_stride >= n N a horizon split anywhere into two chained calls -- the later part's gq0, gdq0 are the
 * earlier part's end seeds -- gives bitwise the single call's result, running seeds or not.  gtau_step_stride = 0 (the sum over the
 * steps) is for a single call.
 * Up to RDYN_MAX_SWEPT_JOINTS input joints (longer chains through their rigid-body reduction): ONE launch for the horizon, lambda in
 * registers between the steps; the workspace query returns 0.  More input joints: CORRECT, NOT FAST -- a host loop over steps and
 * stages on the batch's stream (the chunked product above, the chunked forward dynamics for the RK4 stage rebuild, one element-wise
 * kernel); state, stage and seed buffers live in the workspace behind the images; results do not depend on chunk_samples;
 * RDYN_ERR_UNSUPPORTED where rdyn_joint_torque_derivatives answers so.
 * Errors, all RDYN_ERR_INVALID_ARGUMENT before any device work: a NULL descriptor; the forward call's errors for n_steps, dt,
 * integrator and tau; a NULL trajectory pointer with T >= 2; traj_step_stride (T >= 2), gtraj_step_stride (with running seeds) or a
 * non-zero gtau_step_stride (with gtau) below n N; gq0, gdq0 and gtau all NULL with samples; the component-list rules; a negative
 * chunk_samples; a workspace smaller than the query's answer.  n_samples = 0 is RDYN_OK.  No allocation, no synchronisation: capturable
 * into a graph once the chain has been used on the device. */
typedef struct rdyn_rollout_adjoint_desc
{
  int32_t n_steps, integrator;       /* as in the forward call                                                                  */
  double dt;
  const double* tau;                 /* the forward call's torques                                                              */
  int64_t tau_step_stride;
  const double* q_traj;              /* the forward call's trajectory with traj_every = 1: record k = x_{k+1}; records           */
  const double* dq_traj;             /*   0 .. T - 2 are read                                                                   */
  int64_t traj_step_stride;
  const double* gq_end;              /* dL/dx_T; each may be NULL (= 0)                                                         */
  const double* gdq_end;
  const double* gq_traj;             /* optional running seeds: record k = dL/dx_{k+1}, k < T                                   */
  const double* gdq_traj;
  int64_t gtraj_step_stride;
  double* gq0;                       /* dL/dx_0; each may be NULL; may alias gq_end / gdq_end                                   */
  double* gdq0;
  double* gtau;                      /* may be NULL; step t at + t * gtau_step_stride (>= n N), 0 = the sum over the steps      */
  int64_t gtau_step_stride;
  int32_t* status;                   /* may be NULL                                                                             */
} rdyn_rollout_adjoint_desc;
size_t rdyn_rollout_adjoint_workspace_bytes(const rdyn_chain* chain, const rdyn_rollout_adjoint_desc* desc, int64_t n_samples,
                                            int64_t chunk_samples);
int rdyn_rollout_adjoint(const rdyn_chain* chain, const rdyn_batch* batch, const rdyn_rollout_adjoint_desc* desc,
                         const rdyn_component* comps, int n_comps, int64_t chunk_samples, void* workspace, size_t workspace_bytes);

/* Adjoint of a rollout WITH the gradients with respect to the model's parameters (no reference counterpart): what loss.backward()
 * through a rollout needs for output-error identification.  Everything rdyn_rollout_adjoint writes for the same descriptor this call
 * writes with the same bits; gq0, gdq0 and gtau may all be NULL here.  The new outputs, selected by rdyn_parameter_gradient:
 *     gpi[P]    P = 10 joints_number, the order of rdyn_nominal_parameters      gcomp[K]   K = rdyn_components_columns, column order
 * = the sum, over the samples whose FINAL status is 1, of the one-evaluation products of rdyn_forward_dynamics_parameter_vjp
 * (pi_bar = -Y' w, comp_bar = -C' w, w = M^-1 seed) at the very seeds the adjoint uses: semi-implicit Euler one product per step at
 * (x_t, tau_t; mu); RK4 four per step, at (X_i, tau_t; kv_i), i = 4 .. 1.  A sample with status -1 contributes NOTHING, not even from
 * the backward steps before it failed.  accumulate = 0 overwrites gpi / gcomp, 1 adds to what is there: a horizon split into two
 * chained calls, the second with accumulate = 1, gives the single call's gpi to rounding (not bitwise: the order of the additions
 * differs).  T = 0 gives zeros (accumulate = 1: leaves the outputs as they are).  gpi and gcomp are reproducible bit for bit from run to
 * run: every lane adds into its own accumulators (element-major in the workspace, [10 n_swept + K][n_samples]) and one fixed-order
 * reduction follows; no floating-point atomics.  A longer chain with at most RDYN_MAX_SWEPT_JOINTS input joints runs on its reduced
 * companion and the sums are expanded by X_f' on the device.
 * More than RDYN_MAX_SWEPT_JOINTS input joints: RDYN_ERR_UNSUPPORTED, before any device work (rdyn_rollout_adjoint serves such chains;
 * their parameter gradients are the follow-up).
 * Errors, all RDYN_ERR_INVALID_ARGUMENT before any device work: those of rdyn_rollout_adjoint (but for its "every output NULL"); a NULL
 * pg, gpi and gcomp both NULL, accumulate other than 0 or 1; a workspace smaller than the query's answer.  n_samples = 0 is RDYN_OK.
 * No allocation, no synchronisation: capturable into a graph once the chain has been used on the device. */
typedef struct rdyn_parameter_gradient
{
  double* gpi;        /* [10 * joints_number], may be NULL */
  double* gcomp;      /* [rdyn_components_columns], may be NULL */
  int32_t accumulate; /* 0: overwrite, 1: add */
} rdyn_parameter_gradient;
size_t rdyn_rollout_adjoint_parameters_workspace_bytes(const rdyn_chain* chain, const rdyn_rollout_adjoint_desc* desc,
                                                       const rdyn_component* comps, int n_comps, int64_t n_samples, int64_t chunk_samples);
int rdyn_rollout_adjoint_parameters(const rdyn_chain* chain, const rdyn_batch* batch, const rdyn_rollout_adjoint_desc* desc,
                                    const rdyn_component* comps, int n_comps, const rdyn_parameter_gradient* pg, int64_t chunk_samples,
                                    void* workspace, size_t workspace_bytes);

/* Reverse mode through external link wrenches (no reference counterpart): the product of rdyn_forward_dynamics_ext and the adjoint of
 * rdyn_rollout_ext.  Notation as at rdyn_forward_dynamics_ext: FD_E(q, Dq, tau, ext) = FD_c(q, Dq, tau - tau_E(q, ext)), tau_E linear in
 * ext, a function of q and not of Dq; the base link's record never enters.
 *   rdyn_forward_dynamics_vjp_ext   per sample, with w = M^-1 ddq_bar:
 *       ddq     = FD_E(q, Dq, tau, ext), the bits of rdyn_forward_dynamics_ext          tau_bar = w
 *       dq_bar  as in rdyn_forward_dynamics_vjp, at this ddq
 *       q_bar   = -(dtau_dq + diag d tau_c / d q + d tau_E / d q)' w at this ddq
 *       ext_bar = -(d tau_E / d ext)' w
 *     ext_bar has exactly the shape and layout of ext->w: links_number x 6 per sample for link = -1, 6 per sample for link >= 0, in the
 *     record layout of the batch; the base link's record is +0.0.  It must not overlap an input or another output.  ext->step_stride
 *     is not read.  Every product is optional (all four NULL with samples: RDYN_ERR_INVALID_ARGUMENT); tau_bar may alias ddq_bar.
 *     Status: the rule of rdyn_forward_dynamics_vjp, extended to the wrench entries the sample reads (a non-finite one gives -1; the base
 *     link's record is not read).  A -1 sample gets quiet NaN in every requested output, ext_bar included.
 *   rdyn_rollout_adjoint_ext        the exact transpose of the scheme rdyn_rollout_ext integrates: the step transposes written at
 *     rdyn_rollout_adjoint with vjp replaced by the product above, evaluated with the wrench of step t (w + t * ext->step_stride), held
 *     over the step and taken at each stage's own q; the RK4 stage states are rebuilt with FD_E.  gext (optional, and so is its gw): the
 *     wrench gradient of step t goes to gw + t * step_stride in the shape of one step's wrench record -- with RK4 the sum of the four
 *     stage products of the step.  step_stride = 0: one record, the sum over the steps (what a wrench held over the horizon needs; in a
 *     single call only, like gtau_step_stride = 0).  With a stride >= one record the bitwise split-horizon property of
 *     rdyn_rollout_adjoint holds, gw included.  A -1 sample's gw is NaN from the failing backward step on (step_stride = 0: the whole
 *     record); nothing is added to another sample.  Every lane adds into its own record in a fixed order, no floating-point atomics:
 *     gw is reproducible bit for bit.  gq0, gdq0, gtau and gw all NULL with samples is RDYN_ERR_INVALID_ARGUMENT.
 * Routing, decided before any device work:
 *   ext == NULL or ext->w == NULL   IS rdyn_forward_dynamics_vjp / rdyn_rollout_adjoint: the same kernels, the same bits, every chain
 *                                   those serve; the queries equal the base queries.  A non-NULL ext_bar / gw is then
 *                                   RDYN_ERR_INVALID_ARGUMENT.
 *   with wrenches, at most RDYN_MAX_SWEPT_JOINTS chain joints: ONE launch for one product or one horizon; the queries return 0.
 *   with wrenches, every chain for which rdyn_forward_dynamics_ext takes the chunked route (more than RDYN_MAX_SWEPT_JOINTS input joints,
 *                                   and long chains that otherwise run on a reduced companion): RDYN_ERR_UNSUPPORTED.  Their reverse
 *                                   mode with wrenches is the follow-up; without wrenches these calls serve them as the base calls do.
 * Errors, all RDYN_ERR_INVALID_ARGUMENT before any device work: those of rdyn_forward_dynamics_vjp / rdyn_rollout_adjoint, those of
 * rdyn_forward_dynamics_ext / rdyn_rollout_ext (the link range; in the adjoint the wrench step_stride rule), and a non-zero
 * gext->step_stride that is negative or smaller than one step's record.  n_samples = 0 is RDYN_OK.  No allocation, no synchronisation:
 * capturable into a graph once the chain has been used on the device. */
size_t rdyn_forward_dynamics_vjp_ext_workspace_bytes(const rdyn_chain* chain, const rdyn_ext_wrenches* ext, int64_t chunk_samples);
int rdyn_forward_dynamics_vjp_ext(const rdyn_chain* chain, const rdyn_batch* batch, const rdyn_component* comps, int n_comps,
                                  const rdyn_ext_wrenches* ext, const double* tau, const double* ddq_bar, double* q_bar, double* dq_bar,
                                  double* tau_bar, double* ext_bar, double* ddq, int32_t* status, int64_t chunk_samples, void* workspace,
                                  size_t workspace_bytes);
typedef struct rdyn_ext_wrench_gradient
{
  double* gw;           /* may be NULL; step t at gw + t * step_stride, one step's wrench record each */
  int64_t step_stride;  /* in doubles; 0 = one record, the sum over the steps */
} rdyn_ext_wrench_gradient;
size_t rdyn_rollout_adjoint_ext_workspace_bytes(const rdyn_chain* chain, const rdyn_rollout_adjoint_desc* desc, const rdyn_ext_wrenches* ext,
                                                int64_t n_samples, int64_t chunk_samples);
int rdyn_rollout_adjoint_ext(const rdyn_chain* chain, const rdyn_batch* batch, const rdyn_rollout_adjoint_desc* desc,
                             const rdyn_component* comps, int n_comps, const rdyn_ext_wrenches* ext, const rdyn_ext_wrench_gradient* gext,
                             int64_t chunk_samples, void* workspace, size_t workspace_bytes);

/* Adjoint of a closed-loop rollout (no reference counterpart): the exact transpose of the scheme rdyn_rollout_feedback integrates, the
 * PD law and its clamp included -- what gain tuning and the optimisation of references with a cost on the control effort need.  Notation
 * of rdyn_rollout_feedback and rdyn_rollout_adjoint.  At an evaluation in step t at the state (q, v):
 *     u_raw = fma(kd, Dq_ref_t - v, fma(kp, q_ref_t - q, tau_ff_t)),   u = clamp(u_raw, +-lim),   a = FD_E(q, v, u, ext_t)
 * Let (q_bar, v_bar, tau_bar) = vjp_E(q, v, u; seed) be the product of rdyn_forward_dynamics_vjp_ext (rdyn_forward_dynamics_vjp without
 * wrenches) taken at the command u; u is formed again in the backward sweep by the forward kernel's own text and carries its bits.  The
 * mask follows the branch the forward call took: m_j = 1 where neither u_raw > lim nor u_raw < -lim (exactly at a limit the law passes
 * through), 0 where clamped; sgn_j = +-1 on the clamped side, else 0.  The mask is a select, not a product: a clamped entry contributes
 * +0.0.  With tot = tau_bar_total + gu (gu: the optional seed on the step's command record, below) and g = m o tot, per joint, in this
 * order and with these roundings on every path:
 *     q_bar = fma(-kp, g, q_bar)         v_bar = fma(-kd, g, v_bar)   (only with kd)           gtau_ff_t += g
 *     gkp   = fma(q_ref_t - q, g, gkp)   gkd   = fma(Dq_ref_t - v, g, gkd)                     glim += sgn o tot
 * and, once the step's gtau_ff_t is complete,   gq_ref_t = kp o gtau_ff_t,   gdq_ref_t = kd o gtau_ff_t   (kp, kd do not depend on the stage).
 *   hold = 0 (the continuous law): this is applied at every product of the step -- RK4 stages 4 .. 1, each at its own rebuilt stage
 *       state X_i, tau_bar_total that product's tau_bar; gu joins at the step's first evaluation only (stage 1).  The corrected
 *       (q_bar, v_bar) enter X_bar_i exactly as the uncorrected ones do in rdyn_rollout_adjoint, g takes tau_bar's place in gtau_t.  The
 *       stage rebuild forms the command anew at each stage state, as the forward call does.
 *   hold = 1 (the digital controller): u = law(x_t) serves the stage rebuild and all four products; tau_bar_total is the sum of the four
 *       stage tau_bars (rdyn_rollout_adjoint's gtau_t); the correction is applied once, at x_t, to lambda_t after the step's products.
 * Semi-implicit Euler has one evaluation per step and is written once: the two modes give the same bits, as the forward call promises.
 * Outputs.  desc->gtau is the gradient with respect to the FEED-FORWARD sequence (per step, or its sum with gtau_step_stride = 0); gq0,
 * gdq0, the status, the running state seeds and gext keep the meaning they have in rdyn_rollout_adjoint_ext.  rdyn_feedback_gradient
 * selects the law's gradients:
 *     gq_ref, gdq_ref   step t at + t * gref_step_stride, addressed like batch->q; gref_step_stride = 0: one record, the sum over the
 *                       steps (the gradient of a constant set point)
 *     gkp, gkd, glim    n per SAMPLE, addressed like batch->q, summed over the steps -- ALWAYS per-sample rows, also when the forward call
 *                       used shared gains (gains_per_sample = 0) and for the always-shared limits: the caller sums the rows over the
 *                       samples.  A device-side reduction is deliberately out of scope.
 *     gu_traj           optional seeds on the command record (fb->tau_traj of the forward call with traj_every = 1): record t =
 *                       dL/d(command of step t's first evaluation), at + t * gu_step_stride
 * Accumulation: every lane adds into its own record in memory, in the order of the backward sweep; no floating-point atomics, the same
 * bits every run.  accumulate = 0 starts gkp, gkd, glim and the gref_step_stride = 0 sums from zero; 1 continues adding to what is there.
 * Split horizons: a horizon split anywhere into two chained calls -- the later part first with accumulate = 0, then the earlier part
 * with accumulate = 1, seeded by the later part's gq0 / gdq0, the later part's references (and gu_traj, torques, wrenches) starting at
 * + t0 * their step strides -- gives the bits of the single call for EVERY output, gkp, gkd, glim included: the additions happen in the
 * same order.
 * Routing, decided before any device work:
 *   fb == NULL   IS rdyn_rollout_adjoint_ext: the same kernels, the same bits, the same workspace query.  A non-NULL gfb with any
 *                output or gu_traj in it is then RDYN_ERR_INVALID_ARGUMENT.
 *   fb given     a chain is served when rdyn_rollout_feedback runs it in registers: at most RDYN_MAX_SWEPT_JOINTS chain joints, and
 *                longer chains with at most that many input joints on their reduced companion when there are no wrenches.  ONE launch
 *                for the horizon; the workspace query returns 0.
 *   fb given and rdyn_rollout_feedback takes the chunked route for the chain: RDYN_ERR_UNSUPPORTED.
 *                The adjoint of the chunked closed loop is the follow-up.  The parameter gradients of the closed loop come from
 *                rdyn_rollout_adjoint_feedback_parameters (below).
 * Status: the rule of rdyn_rollout_adjoint_ext, extended to the references, gains and limits the sample reads: a non-finite entry gives
 * -1.  From the failing backward step on every output of the sample is quiet NaN -- its reference gradients of that step and the earlier
 * ones, and its whole gkp / gkd / glim rows and summed reference gradients.  No sample affects another.
 * T = 0 copies the end seeds; with accumulate = 0 it writes zeros to the sums, with accumulate = 1 it leaves them as they are.
 * Errors, all RDYN_ERR_INVALID_ARGUMENT before any device work: those of rdyn_rollout_adjoint_ext; those of rdyn_rollout_feedback
 * concerning fb (NULL q_ref or kp, the ref_step_stride rule, hold or gains_per_sample outside {0, 1}); gkd or gdq_ref without fb->kd; glim
 * without fb->tau_limit; a negative gref_step_stride or a non-zero one below n N (with gq_ref or gdq_ref); gu_traj with a gu_step_stride
 * below n N; accumulate outside {0, 1}; gq0, gdq0, gtau, gw and every output of gfb NULL with samples.  n_samples = 0 is RDYN_OK.  No
 * allocation and no synchronisation: capturable into a graph once the chain has been used on the device. */
typedef struct rdyn_feedback_gradient
{
  double* gq_ref;            /* optional; step t at + t * gref_step_stride, addressed like batch->q */
  double* gdq_ref;           /* optional, likewise; needs fb->kd */
  int64_t gref_step_stride;  /* 0 = one record: the sum over the steps (a constant set point); otherwise >= n N */
  double* gkp;               /* optional; n per SAMPLE, addressed like batch->q, summed over the steps */
  double* gkd;               /* optional, likewise; needs fb->kd */
  double* glim;              /* optional, likewise; needs fb->tau_limit */
  int32_t accumulate;        /* 0: overwrite; 1: continue adding to what is there (gkp, gkd, glim, the stride-0 sums) */
  const double* gu_traj;     /* optional seeds on the command record: record t = dL/d(command of step t's first evaluation) */
  int64_t gu_step_stride;    /* >= n N when gu_traj is given */
} rdyn_feedback_gradient;
size_t rdyn_rollout_adjoint_feedback_workspace_bytes(const rdyn_chain* chain, const rdyn_rollout_adjoint_desc* desc,
                                                     const rdyn_ext_wrenches* ext, const rdyn_feedback* fb, int64_t n_samples,
                                                     int64_t chunk_samples);
int rdyn_rollout_adjoint_feedback(const rdyn_chain* chain, const rdyn_batch* batch, const rdyn_rollout_adjoint_desc* desc,
                                  const rdyn_component* comps, int n_comps, const rdyn_ext_wrenches* ext,
                                  const rdyn_ext_wrench_gradient* gext, const rdyn_feedback* fb, const rdyn_feedback_gradient* gfb,
                                  int64_t chunk_samples, void* workspace, size_t workspace_bytes);

/* Adjoint of a closed-loop rollout WITH the gradients with respect to the model's parameters (no reference counterpart): what
 * loss.backward() through the simulated closed loop needs for output-error identification of a robot that is only ever excited under
 * its controller.  It is rdyn_rollout_adjoint_feedback and rdyn_rollout_adjoint_parameters in one sweep.
 * Outputs shared with rdyn_rollout_adjoint_feedback: for the same descriptor, law and selection this call writes the same bits in gq0,
 * gdq0, gtau, the status and the law's gradients gq_ref, gdq_ref, gkp, gkd and glim, gu_traj seeds and gfb->accumulate included.  gfb may
 * be NULL or empty, and gq0, gdq0, gtau may all be NULL: gpi or gcomp is an output.
 * gpi and gcomp are defined as at rdyn_rollout_adjoint_parameters: the sum, over the samples whose FINAL status is 1, of the
 * one-evaluation products pi_bar = -Y' w and comp_bar = -C' w with w = M^-1 seed, taken at the very seeds the closed-loop adjoint uses:
 * semi-implicit Euler one product per step at (x_t, u_t; mu); RK4 four per step at (X_i, u; kv_i), i = 4 .. 1.  u is the command the
 * forward call applied there: under hold = 1, and for semi-implicit Euler, the held command of the step; under hold = 0 with RK4 the
 * command formed at the stage state.  w is the product's tau_bar BEFORE the law's transpose masks it.  The law does not depend on the
 * model, so there is no further term.
 * Reproducibility and accumulation: gpi and gcomp are reproducible bit for bit from run to run (every lane adds into its own
 * accumulators, element-major in the workspace, [10 n_swept + K][n_samples]; one fixed-order reduction follows; no floating-point
 * atomics).  A sample with status -1 contributes NOTHING to gpi / gcomp, not even from the backward steps before it failed, and is NaN in
 * its own rows of the other outputs only.  pg->accumulate and gfb->accumulate are independent flags.  A horizon split into two chained
 * calls, the earlier part with both flags 1, gives the single call's bits in the state and law gradients and its gpi / gcomp to rounding.
 * T = 0: what rdyn_rollout_adjoint_feedback does, and zeros in gpi / gcomp (pg->accumulate = 1: leaves them as they are).
 * Routing, decided before any device work:
 *   fb == NULL and no wrenches   IS rdyn_rollout_adjoint_parameters: the same kernels, the same bits, the same workspace query.  A gfb
 *                with any output or gu_traj in it is then RDYN_ERR_INVALID_ARGUMENT.
 *   ext with w != NULL           RDYN_ERR_UNSUPPORTED: the parameter gradients with external wrenches are the next step; ext and gext are
 *                in the signature so that it need not change then.  The query returns 0.
 *   fb given and rdyn_rollout_feedback takes the chunked route for the chain: RDYN_ERR_UNSUPPORTED, as at rdyn_rollout_adjoint_feedback.
 *   otherwise    at most RDYN_MAX_SWEPT_JOINTS chain joints, and longer chains with at most that many input joints on their reduced
 *                companion, the sums expanded by X_f' on the device: ONE launch for the horizon plus the reduction of
 *                rdyn_rollout_adjoint_parameters; the workspace is that call's.
 * Errors, all RDYN_ERR_INVALID_ARGUMENT before any device work: those of rdyn_rollout_adjoint_feedback and those of
 * rdyn_rollout_adjoint_parameters; "every output NULL" cannot occur, since a NULL pg, or one with gpi and gcomp both NULL, is invalid as
 * in the open-loop call.  n_samples = 0 is RDYN_OK.  No allocation and no synchronisation: capturable into a graph once the chain has
 * been used on the device. */
size_t rdyn_rollout_adjoint_feedback_parameters_workspace_bytes(const rdyn_chain* chain, const rdyn_rollout_adjoint_desc* desc,
                                                                const rdyn_component* comps, int n_comps, const rdyn_ext_wrenches* ext,
                                                                const rdyn_feedback* fb, int64_t n_samples, int64_t chunk_samples);
int rdyn_rollout_adjoint_feedback_parameters(const rdyn_chain* chain, const rdyn_batch* batch, const rdyn_rollout_adjoint_desc* desc,
                                             const rdyn_component* comps, int n_comps, const rdyn_ext_wrenches* ext,
                                             const rdyn_ext_wrench_gradient* gext, const rdyn_feedback* fb,
                                             const rdyn_feedback_gradient* gfb, const rdyn_parameter_gradient* pg, int64_t chunk_samples,
                                             void* workspace, size_t workspace_bytes);

/* ---- mixed-chain batch (BASELINE.json configs[4]: 256 distinct 6-7-DOF chains x 4 096 samples) --------------
 * One launch per group of chains with equal joint count (and output-layout kind) evaluates rdyn_regressor for MANY
 * (chain, batch) items: grid = (ceil(max samples / workgroup), items); every workgroup reads its item's descriptor and its
 * chain's constants through scalar loads.  Items in the per-sample image or the stacked layout (rdyn_regressor_layout presets)
 * take the same LDS-staged whole-line kernels as rdyn_regressor; any other strides the strided one.  A plan freezes the items (device pointers, layouts) so that running it allocates and
 * copies nothing (graph-capturable).  All items must live on the same device (items[0].batch.device).  A plan holds the
 * device copies of its chains' constants: the chains must outlive the plan and must not be re-configured
 * (rdyn_chain_set_input_joints) while it exists. */
typedef struct rdyn_multi_item
{
  const rdyn_chain* chain;
  rdyn_batch batch;              /* stream field ignored */
  double* tau;                   /* may be NULL */
  double* Y;
  rdyn_regressor_layout y_layout;
} rdyn_multi_item;
typedef struct rdyn_multi_plan rdyn_multi_plan;
int rdyn_multi_plan_create(const rdyn_multi_item* items, int n_items, rdyn_multi_plan** out);
int rdyn_multi_plan_regressor(const rdyn_multi_plan* plan, void* stream);
void rdyn_multi_plan_destroy(rdyn_multi_plan* plan);

/* ---- normal equations of the stacked regressor (fp64 MFMA) ------------------------------------------------
 * No counterpart inside rosdyn_core: the identification step that stacked getRegressor rows and solved the
 * least-squares problem lived in the external rosdyn_identification (top-level README.md:15).  BASELINE.json's
 * north star asks for the Gram reduction on the matrix cores, so it is part of this boundary.
 *
 * rdyn_gram: A is any column-major rows x n_cols DEVICE matrix (leading dimension lda >= rows), b a DEVICE
 * vector of `rows` doubles or NULL.  Writes (accumulate == 0) or adds (accumulate != 0)
 *   G  = A^T A   n_cols x n_cols column-major, both triangles      (device)
 *   c  = A^T b   n_cols                                             (device, may be NULL)
 *   bb = b^T b   1                                                  (device, may be NULL)
 * with v_mfma_f64_16x16x4_f64; bitwise reproducible (fixed summation order, no atomics).
 * workspace: rdyn_gram_workspace_bytes(n_cols) bytes of device memory. */
size_t rdyn_gram_workspace_bytes(int n_cols);
int rdyn_gram(const double* A, int64_t rows, int64_t lda, int n_cols, const double* b, double* G, double* c, double* bb,
              int accumulate, void* workspace, size_t workspace_bytes, int device, void* stream);

/* rdyn_regressor_gram: G, c, bb of the stacked regressor A (N*n x P) of the batch and measured torques
 * tau_meas (same layout as batch->q) WITHOUT leaving the regressor in HBM: the batch is processed in chunks of
 * `chunk_samples` (0 = default 32768) whose element-major regressor image (chunk * n * (P + 1) doubles, reused
 * for every chunk, sized to stay resident in the 256 MiB Infinity Cache) is produced by the regressor kernel
 * and consumed by the Gram kernel.  Multi-GPU: every rank calls this on its shard and all-reduces
 * [G | c | bb] (P*P + P + 1 doubles) once -- rosdyn_amd/gram.py. */
/* The identification step in one call: normal equations of the stacked [Y | C] with the measured torque,
 *   G = [Y C]'[Y C]  ((P + K) x (P + K)),  c = [Y C]' tau_meas,  bb = tau_meas' tau_meas,
 * Y = getRegressor of the chain (P = 10 joints_number columns), C = the component columns of rdyn_components_regressor
 * (K = rdyn_components_columns; n_comps = 0: none).  Neither Y nor C is handed to the caller: they are produced chunk by
 * chunk into the workspace and reduced by the MFMA Gram kernel.  P + K <= 111.  Outputs / accumulate as rdyn_regressor_gram. */
size_t rdyn_identification_gram_workspace_bytes(const rdyn_chain* chain, const rdyn_component* comps, int n_comps);
int rdyn_identification_gram(const rdyn_chain* chain, const rdyn_component* comps, int n_comps, const rdyn_batch* batch,
                             const double* tau_meas, double* G, double* c, double* bb, int accumulate, void* workspace,
                             size_t workspace_bytes);
size_t rdyn_regressor_gram_workspace_bytes(const rdyn_chain* chain, int64_t chunk_samples);
int rdyn_regressor_gram(const rdyn_chain* chain, const rdyn_batch* batch, const double* tau_meas, double* G, double* c,
                        double* bb, int accumulate, int64_t chunk_samples, void* workspace, size_t workspace_bytes);

/* ---- normal equations wider than 111 columns (column-panel fp64-MFMA Gram, rdyn_panel_gram.hip) ----------------------------
 * rdyn_gram_wide: rdyn_gram for up to RDYN_MAX_WIDE_COLUMNS columns (always the panel kernel, whatever the width): the columns of
 * [A | b] are cut into panels of 64 and one launch reduces every panel pair.  Same outputs, accumulate and determinism as rdyn_gram;
 * workspace: rdyn_gram_wide_workspace_bytes(n_cols) bytes (0 unless 1 <= n_cols <= RDYN_MAX_WIDE_COLUMNS).
 * rdyn_regressor_gram_wide / rdyn_identification_gram_wide: rdyn_regressor_gram / rdyn_identification_gram for every chain the library
 * ingests -- up to RDYN_MAX_JOINTS chain joints, any number of input joints in any order, fixed joints anywhere, up to 30 components --
 * as long as 10 joints_number + K <= RDYN_MAX_WIDE_COLUMNS.  A request the narrow call serves is handed to it (the workspace query
 * then returns the narrow call's size); the rest goes through element-major chunk images of [Y | C | tau_meas] (chunk_samples per
 * chunk; 0 = as many as keep one image within 128 MiB, at least 16 384) into the panel kernel, chains with
 * fixed joints and at most RDYN_MAX_SWEPT_JOINTS input joints through their reduced companion.  Outputs, accumulate, N = 0 and
 * NULL c / bb as rdyn_regressor_gram; no allocation, no synchronisation (graph-capturable).  RDYN_ERR_INVALID_ARGUMENT for null or
 * undersized arguments (before any device work), RDYN_ERR_UNSUPPORTED only past RDYN_MAX_WIDE_COLUMNS columns. */
#define RDYN_MAX_WIDE_COLUMNS 415
size_t rdyn_gram_wide_workspace_bytes(int n_cols);
int rdyn_gram_wide(const double* A, int64_t rows, int64_t lda, int n_cols, const double* b, double* G, double* c, double* bb,
                   int accumulate, void* workspace, size_t workspace_bytes, int device, void* stream);
size_t rdyn_regressor_gram_wide_workspace_bytes(const rdyn_chain* chain, int64_t chunk_samples);
int rdyn_regressor_gram_wide(const rdyn_chain* chain, const rdyn_batch* batch, const double* tau_meas, double* G, double* c,
                             double* bb, int accumulate, int64_t chunk_samples, void* workspace, size_t workspace_bytes);
size_t rdyn_identification_gram_wide_workspace_bytes(const rdyn_chain* chain, const rdyn_component* comps, int n_comps,
                                                     int64_t chunk_samples);
int rdyn_identification_gram_wide(const rdyn_chain* chain, const rdyn_component* comps, int n_comps, const rdyn_batch* batch,
                                  const double* tau_meas, double* G, double* c, double* bb, int accumulate,
                                  int64_t chunk_samples, void* workspace, size_t workspace_bytes);

/* ---- BASELINE.json configs[3] inside the library (rdyn_multi_gpu.cpp): one process, the trajectory batch
 * sharded over the GPUs of a node, every GPU the fused regressor -> Gram of its shard, then ONE
 * ncclAllReduce(P*P + P + 2 doubles, ncclDouble, ncclSum) over RCCL / xGMI.  rdyn_multi_gpu_create initialises one communicator
 * (ncclCommInitAll) and one stream per device; RCCL is resolved at run time (the library named by RDYN_RCCL_PATH if that variable is
 * set, else librccl.so.1) -> RDYN_ERR_UNSUPPORTED if absent.
 * rdyn_regressor_gram_multi: batches[i] (device pointers on devices[i]; batch.device = devices[i] or -1), tau_meas[i] (may be NULL
 * as a whole or per shard), acc[i] = a device buffer of P*P + P + 2 doubles on devices[i].  The work runs on the CONTEXT's stream of
 * each device, ordered BEHIND everything already queued on batches[i].stream (NULL = that device's default stream) by an event, so
 * inputs still being produced there are safe; results are ordered for the caller by rdyn_multi_gpu_synchronize (or a device
 * synchronise).  Calls may be queued back to back without synchronising in between (the shard size is a kernel argument, nothing
 * host-side is re-used).  On completion
 * EVERY acc[i] holds the sums over all shards  [G = A'A (P*P, column-major) | c = A'tau_meas (P) | bb = tau_meas'tau_meas | count].
 * No reference counterpart (rosdyn_core has no multi-device code). */
typedef struct rdyn_multi_gpu rdyn_multi_gpu;
int rdyn_multi_gpu_create(const int* devices, int n_devices, rdyn_multi_gpu** out);
void rdyn_multi_gpu_destroy(rdyn_multi_gpu* ctx);
int rdyn_multi_gpu_device_count(const rdyn_multi_gpu* ctx);
int rdyn_multi_gpu_synchronize(rdyn_multi_gpu* ctx);
int rdyn_regressor_gram_multi(rdyn_multi_gpu* ctx, const rdyn_chain* chain, const rdyn_batch* batches, const double* const* tau_meas,
                              double* const* acc);
/* The same with accumulate != 0: acc[i] <- acc[i] + the sums over all shards of THIS call (a batch streamed through the devices in
 * pieces: the first piece with accumulate = 0, the others with 1; the accumulators hold the same totals on every device before and
 * after).  One ncclAllReduce per call either way.  The per-device part of both calls is issued by one host thread per device.
 * Failures: everything that can be refused (null pointers, devices, the chain's width) is checked BEFORE anything is queued; if a
 * device fails later (a launch or allocation error on one shard) the call returns that device's error WITHOUT issuing the collective,
 * and the other devices have already queued kernels that overwrite their outputs with their OWN shard's sums / factor: treat every
 * acc[i] / R1[i] of a failed call as undefined.  A collective that fails half-way aborts the communicators (and closes the RCCL group
 * it was issued in): the context then only accepts rdyn_multi_gpu_destroy; a new context can be created from the same thread. */
int rdyn_regressor_gram_multi_accumulate(rdyn_multi_gpu* ctx, const rdyn_chain* chain, const rdyn_batch* batches, const double* const* tau_meas,
                                         double* const* acc, int accumulate);
/* The R factor WITHOUT the normal equations over the devices of the context (the TSQR alternative):
 * device i computes the robust factor of its shard (rdyn_identification_tsqr with all its routes; comps may be NULL / n_comps 0:
 * rdyn_regressor_tsqr), ONE ncclAllGather moves the factors of the SWEPT chain (the reduced companion of a chain with joints that are
 * not input joints: at most 112 columns whatever the chain's own width -- the payload of the Gram all-reduce or less), every device
 * folds the same stack in the same fixed order and expands the result: on completion EVERY R1[i] (device i, n1 x n1 column-major,
 * n1 = 10 joints_number + K + 1) holds the factor of all shards, bitwise identical on all devices.  Every chain the single-device
 * entry point serves is served.  If a collective fails half-way the communicators are aborted and the context only accepts
 * rdyn_multi_gpu_destroy.  accumulate != 0: R1[i] <- factor of [previous R1[i] ; all shards].
 * Asynchronous like rdyn_regressor_gram_multi.  Both calls end by making batches[i].stream WAIT (on the device, by an event) for the
 * collective: work queued on the caller's stream afterwards sees the results; a host-side read still needs a synchronisation
 * (rdyn_multi_gpu_synchronize, or of that stream). */
int rdyn_identification_tsqr_multi(rdyn_multi_gpu* ctx, const rdyn_chain* chain, const rdyn_component* comps, int n_comps,
                                   const rdyn_batch* batches, const double* const* tau_meas, double* const* R1, int accumulate);
int rdyn_regressor_tsqr_multi(rdyn_multi_gpu* ctx, const rdyn_chain* chain, const rdyn_batch* batches, const double* const* tau_meas,
                              double* const* R1, int accumulate);

/* ---- tall-skinny QR (rdyn_tsqr.hip): the R factor of [A | b] WITHOUT forming A'A -- BASELINE.json configs[2] "regressor + TSQR".
 * The Gram route squares the condition number; this one does not.  Every wave folds row blocks into a running upper-triangular
 * factor by Householder reflections (R <- qr([R; block])), the factors are folded pairwise, level by level, in a fixed
 * order (bitwise reproducible).  Output R1, DEVICE, column-major n1 x n1 with n1 = n_cols + (b != NULL):
 *   R1 = [R d; 0 rho],  A = Q R,  d = Q'b,  rho = |A x_ls - b|   (diagonal signs are not normalised)
 * accumulate != 0: R1 <- factor of [previous R1 ; new rows] (chunked batches).  Multi-GPU: every rank all-gathers its R1 and folds
 * the stack with rdyn_tsqr_combine_host.  Solve with rdyn_solve_r_factor(R1, n1, n_cols, n_cols, d = R1 + n_cols * n1, ...).
 * rdyn_tsqr: any column-major rows x n_cols device matrix, n1 <= 112 (what rdyn_gram takes: a materialised [Y | C | tau_meas] of a
 * chain with fixed frames and friction columns has 90 - 110 columns).  rdyn_regressor_tsqr: the stacked regressor of the batch and
 * tau_meas (layout of batch->q), n1 = 10 joints_number + 1; chains of 1..10 INPUT joints in any order; joints that are not input
 * joints are folded away (the reduced chain of rdyn_chain_reduction is swept and the factor expanded by a small QR: up to
 * RDYN_MAX_JOINTS chain joints).  Up to 8 input joints the rows are generated in LDS by the regressor sweep and never stored (input
 * joints listed out of chain order: the kernels sweep in chain order and read q, Dq, DDq, tau_meas of every row through an index map
 * -- A'A, A'tau and R do not depend on the order of the rows inside a sample); 9..10 input joints: chunk images of 65 536 samples in
 * the workspace (65 536 x n x (10 n + 1) doubles: 0.43 GB at 9, 0.53 GB at 10 input joints -- per device in the multi-device form;
 * size buffers with rdyn_regressor_tsqr_workspace_bytes, never from a figure in a comment) factored by rdyn_tsqr's kernels.
 * rdyn_identification_tsqr: the same for the identification step's [Y | C | tau_meas] (C = the component columns of
 * rdyn_components_regressor -- friction_polynomial1.h:126, ideal_spring.h:64 -- K = rdyn_components_columns):
 * n1 = 10 joints_number + K + 1 <= 112 after the reduction, unknowns [inertial ; component] parameters.  The component columns
 * belong to input joints and pass through the reduction unchanged, so the reference's own chains (ur10 base_link -> tool0,
 * test.cpp:47-48; a Panda with its fixed flange and hand frames) are served with friction columns stacked beside getRegressor.
 * Routes, chosen by the shape and the batch size:
 *   Householder folds on the vector units -- in the registers of one wave where the factor fits them (rdyn_tsqr.hip: <= 64 columns of a
 *     matrix; swept chains of 2..7 joints, 2..6 with component columns; ~5x the time of rdyn_regressor_gram), with the factor packed in
 *     LDS beyond (rdyn_tsqr_wide.hip: up to 112 columns; a 7-joint arm with friction columns; slower, a dependent chain per column);
 *   from 4 096 samples (32 768 rows of a matrix) on, factors of <= 96 columns (rdyn_tsqr on a matrix: <= 112): preconditioned CholeskyQR with the heavy pass on the
 *     fp64 matrix cores (rdyn_cholqr.hip: a triangular T from the Gram matrix of a row subsample, W = T^-1 with nearly dependent
 *     pivots deferred, G2 = (A W)'(A W) over all rows by MFMA, R = chol(G2) T; the device accepts the result only if the measured
 *     error growth of A W and the conditioning of the equilibrated A W are small, runs a second round from R otherwise, and falls
 *     back to the Householder folds of all rows if that is not accepted either -- all inside the one asynchronous call; ~1.7x the
 *     time of rdyn_regressor_gram; rows of R at structurally dependent columns are exactly zero).
 * Every route returns R1 with R1'R1 = [A b]'[A b] to rounding and the small singular values to ~cond * eps.
 * The first call per (chain, device) uploads the chain's constants (a blocking copy): make it outside a stream capture. */
size_t rdyn_tsqr_workspace_bytes(int n_cols_with_rhs);
int rdyn_tsqr(const double* A, int64_t rows, int64_t lda, int n_cols, const double* b, double* R1, int accumulate, void* workspace,
              size_t workspace_bytes, int device, void* stream);
size_t rdyn_regressor_tsqr_workspace_bytes(const rdyn_chain* chain);
int rdyn_regressor_tsqr(const rdyn_chain* chain, const rdyn_batch* batch, const double* tau_meas, double* R1, int accumulate, void* workspace,
                        size_t workspace_bytes);
size_t rdyn_identification_tsqr_workspace_bytes(const rdyn_chain* chain, const rdyn_component* comps, int n_comps);
int rdyn_identification_tsqr(const rdyn_chain* chain, const rdyn_component* comps, int n_comps, const rdyn_batch* batch, const double* tau_meas,
                             double* R1, int accumulate, void* workspace, size_t workspace_bytes);
/* What the LAST rdyn_regressor_tsqr / rdyn_identification_tsqr call that used `workspace` did (the preconditioned route decides on the
 * device which of its stages vouches for the result; this reads the decision back).  Same chain, components and n_samples as that
 * call; waits for `stream`.  No reference counterpart. */
typedef struct rdyn_tsqr_report
{
  int32_t route;      /* 0: Householder folds (batches below 4 096 samples, shapes the other route does not serve): nothing else is
                         filled in; 1: preconditioned CholeskyQR */
  int32_t stage;      /* route 1: 0 = accepted after round 0, 1 = after round 1, 2 = the stand-by Householder factorisation ran */
  int32_t n_deferred; /* columns the last preconditioner did not use for elimination (structurally dependent or nearly so) */
  int32_t reserved;
  double gamma[2];    /* growth factor of the rounding of A W on the column norms of all rows, round 0 / 1 (0 = round not run);
                         accepted up to 1e4 */
  double rho[2];      /* |Re^-1|_F / sqrt(k) of the column-equilibrated A W (1 = orthogonal columns), round 0 / 1; accepted up to 4 */
} rdyn_tsqr_report;
int rdyn_tsqr_last_report(const rdyn_chain* chain, const rdyn_component* comps, int n_comps, int64_t n_samples, const void* workspace,
                          int device, void* stream, rdyn_tsqr_report* out);
/* the same for the last rdyn_tsqr call (n_cols_with_rhs = n_cols + (b != NULL), rows as in that call) */
int rdyn_tsqr_rows_last_report(int n_cols_with_rhs, int64_t rows, const void* workspace, int device, void* stream, rdyn_tsqr_report* out);
/* ---- R factors wider than 112 columns (preconditioned CholeskyQR over column panels: rdyn_panel_trmm.hip, rdyn_panel_gram.hip, the
 * PANEL dense steps of rdyn_cholqr.hip).  Each call mirrors its narrow counterpart argument for argument (the chain forms + chunk_samples:
 * samples per chunk image, 0 = default, as rdyn_regressor_gram_wide).  R1 (n1 x n1, column-major, upper triangular, n1 = n_cols + 1 with
 * the rhs / tau_meas column, n1 <= RDYN_MAX_WIDE_COLUMNS + 1): R1'R1 = [A b]'[A b]; rows of the directions the factor kernel finds null
 * are exactly zero.  A request the narrow call serves is handed to it, and the workspace query then returns the narrow size.
 * RDYN_ERR_UNSUPPORTED only past the wide limit (chains with fixed joints: also when their reduced companion is narrower than 113
 * columns while the chain is wider), RDYN_ERR_INVALID_ARGUMENT for null or undersized arguments before any device work.  accumulate,
 * N = 0 and tau_meas == NULL as in the narrow calls.  No allocation, no synchronisation: the calls can be captured in a graph.
 * Round 0 builds W = T^-1 from the Gram matrix of a row subsample (every S-th 16-row group of a matrix; one chunk image of every S-th
 * sample of a batch), Q = [A b] W runs on the matrix cores one row chunk / chunk image at a time, R = chol(Q'Q) T; rounds 1 and 2
 * re-precondition with the factor of the round before, started by the device only when that round was not accepted (gamma <= 1e4 and
 * rho <= 4).  There is no Householder stand-by at these widths: when no round is accepted, round 2's factor stands and the report says
 * so (stage 3).  Chains go through chunk images of [Y | C | tau_meas]; chains with fixed joints through the reduced companion, expanded
 * by R = qr(R_red E_aug).  Solve with rdyn_solve_r_factor; fold factors with rdyn_tsqr_combine_host. */
size_t rdyn_tsqr_wide_workspace_bytes(int n_cols_with_rhs);
int rdyn_tsqr_wide(const double* A, int64_t rows, int64_t lda, int n_cols, const double* b, double* R1, int accumulate, void* workspace,
                   size_t workspace_bytes, int device, void* stream);
size_t rdyn_regressor_tsqr_wide_workspace_bytes(const rdyn_chain* chain, int64_t chunk_samples);
int rdyn_regressor_tsqr_wide(const rdyn_chain* chain, const rdyn_batch* batch, const double* tau_meas, double* R1, int accumulate,
                             int64_t chunk_samples, void* workspace, size_t workspace_bytes);
size_t rdyn_identification_tsqr_wide_workspace_bytes(const rdyn_chain* chain, const rdyn_component* comps, int n_comps, int64_t chunk_samples);
int rdyn_identification_tsqr_wide(const rdyn_chain* chain, const rdyn_component* comps, int n_comps, const rdyn_batch* batch,
                                  const double* tau_meas, double* R1, int accumulate, int64_t chunk_samples, void* workspace,
                                  size_t workspace_bytes);
typedef struct rdyn_tsqr_wide_report
{
  int32_t route;      /* 2: column-panel CholeskyQR; 0: the width is served by the narrow calls (read their report) */
  int32_t stage;      /* 0, 1, 2: the round whose factor was accepted; 3: none was, round 2's factor stands */
  int32_t n_deferred; /* columns the last preconditioner did not use for elimination */
  int32_t reserved;
  double gamma[3];    /* growth factor of the rounding of A W, rounds 0..2 (0 = round not run); accepted up to 1e4 */
  double rho[3];      /* |Re^-1|_F / sqrt(k) of the column-equilibrated A W, rounds 0..2; accepted up to 4 */
} rdyn_tsqr_wide_report;
/* What the last wide factor call that used `workspace` did; n_cols_with_rhs = the width of its factor (10 joints_number + K + 1 for the
 * chain forms).  Waits for `stream`. */
int rdyn_tsqr_wide_last_report(int n_cols_with_rhs, const void* workspace, int device, void* stream, rdyn_tsqr_wide_report* out);
/* HOST: folds n_factors upper-triangular n x n factors (stacked, each column-major n x n) into one (Householder). */
int rdyn_tsqr_combine_host(const double* R_stack, int n_factors, int n, double* R_out);

/* ---- the small dense solves of the identification step (HOST pointers, column-major; rdyn_solve.cpp).  No counterpart inside
 * rosdyn_core (external rosdyn_identification, README.md:15).
 * rdyn_solve_normal_equations: minimum-norm least-squares solution x (n) of G x = c for the symmetric positive SEMI-definite
 *   n x n Gram G (the stacked regressor is structurally rank deficient: unobservable base-link parameters, fixed tail links):
 *   Jacobi eigen-decomposition, eigenvalues <= rtol * lambda_max dropped; *rank (may be NULL) = eigenvalues kept.
 * rdyn_gram_r_factor: rank-revealing R factor of A from its Gram: pivoted Cholesky, R'R = G[perm][:, perm]; R is n x n
 *   (rows >= *rank are zero), perm[n].  Squares the condition number (CholeskyQR): fine for cond(A) << 1e8.
 * rdyn_solve_r_factor: minimum-norm solution of min |R x - d| for a rows x n factor R (leading dimension ldr) as the TSQR path
 *   returns it (rdyn_regressor_tsqr below: condition number NOT squared), singular values <= rtol * sigma_max dropped. */
int rdyn_solve_normal_equations(const double* G, const double* c, int n, double rtol, double* x, int* rank);
int rdyn_gram_r_factor(const double* G, int n, double rtol, double* R, int32_t* perm, int* rank);
int rdyn_solve_r_factor(const double* R, int64_t ldr, int rows, int n, const double* d, double rtol, double* x, int* rank);

#ifdef __cplusplus
}
#endif
#endif /* RDYN_H */
