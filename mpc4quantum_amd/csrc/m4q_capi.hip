// m4q_capi.hip - host side of the C ABI declared in include/m4q.h.
// Owns device memory, streams and events; dispatches to the per-shape kernel objects.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <rccl/rccl.h>      // types and prototypes only: librccl.so is loaded with dlopen on first use (a CPU-only import never needs it)

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <complex>
#include <cstdlib>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <deque>
#include <functional>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/m4q.h"
#include "m4q_args.h"
#include "m4q_lift.h"
#include "m4q_robust_host.h"

namespace m4q {
struct cplx { double re, im; };
}
using m4q::cplx;
using m4q::lift::Lift;
using m4q::lift::LiftStat;
using m4q::lift::lift_blocks;
using m4q::lift::lift_vectors;

// per-shape registration functions (m4q_kernels.hip compiled once per shape)
#define M4Q_SHAPE(nx, nu, ord) extern "C" const m4q::ShapeOps* m4q_shape_##nx##_##nu##_##ord();
#include "m4q_shapes.inc"
#undef M4Q_SHAPE

extern "C" __attribute__((visibility("hidden"))) void dim_d_anchor() {}      // an address inside this library, for dladdr

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess) return fail(-(int)e_, "%s: %s", #expr, hipGetErrorString(e_));       \
  } while (0)

// inside m4q_session_create, once the session object exists: a failing HIP call must not leak it
#define HIP_TRY_OWNED(sess, expr)                                                              \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess) {                                                                    \
      m4q_session_destroy(sess);                                                               \
      return fail(-(int)e_, "%s: %s", #expr, hipGetErrorString(e_));                           \
    }                                                                                          \
  } while (0)

// plant_ok: plant-only shapes (m4q_shapes.inc) count too - for m4q_plant_step_batch; every other entry point needs the full set
const m4q::ShapeOps* find_shape(int nx, int nu, int order, bool plant_ok = false) {
  static const m4q::ShapeOps* table[] = {
#define M4Q_SHAPE(nx, nu, ord) m4q_shape_##nx##_##nu##_##ord(),
#include "m4q_shapes.inc"
#undef M4Q_SHAPE
  };
  for (const m4q::ShapeOps* s : table)
    if (s->nx == nx && s->nu == nu && s->order == order && (plant_ok || !s->plant_only)) return s;
  return nullptr;
}

// any compiled order for (nx, nu): the QP and plant kernels do not depend on the library order
const m4q::ShapeOps* find_shape_any_order(int nx, int nu, bool plant_ok = false) {
  for (int ord = 1; ord <= 3; ++ord)
    if (const m4q::ShapeOps* s = find_shape(nx, nu, ord, plant_ok)) return s;
  return nullptr;
}

// The closed-loop kernels with the GENERATOR plant live in a second library, libm4q_hip_gen.so, next to this one (M4Q_GEN_LIB
// overrides the path): loaded the first time a session asks for that plant, never otherwise.  Returns the ops whose launch_mpc /
// occupancy / mpc_lds_bytes serve such a session, or nullptr with the reason in `why`.
const m4q::ShapeOps* gen_shape(int nx, int nu, int order, std::string& why) {
  static std::mutex mu;
  static void* handle = nullptr;
  static std::string load_error;
  std::lock_guard<std::mutex> lock(mu);
  if (!handle && load_error.empty()) {
    std::string path;
    if (const char* env = std::getenv("M4Q_GEN_LIB")) {
      path = env;
    } else {
      Dl_info info{};
      if (dladdr(reinterpret_cast<const void*>(&dim_d_anchor), &info) && info.dli_fname) {
        path = info.dli_fname;
        const size_t slash = path.find_last_of('/');
        path = (slash == std::string::npos ? std::string() : path.substr(0, slash + 1)) + "libm4q_hip_gen.so";
      }
    }
    handle = path.empty() ? nullptr : dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
    if (!handle) {
      const char* err = path.empty() ? nullptr : dlerror();          // (dlerror() clears itself: ask once)
      load_error = "the generator-plant kernels are in libm4q_hip_gen.so, which did not load (" + path + "): " + (err ? err : "?");
    }
  }
  if (!handle) { why = load_error; return nullptr; }
  char name[64];
  snprintf(name, sizeof(name), "m4q_shapeg_%d_%d_%d", nx, nu, order);
  typedef const m4q::ShapeOps* (*fn_t)();
  fn_t fn = reinterpret_cast<fn_t>(dlsym(handle, name));
  if (!fn) { why = std::string("libm4q_hip_gen.so has no ") + name; return nullptr; }
  return fn();
}

int dim_d(int nx) { return nx == 4 ? 2 : nx == 9 ? 3 : nx == 16 ? 4 : 0; }
// d with d^4 = nx (M4Q_PLANT_PROCESS: the process vector of a d x d unitary), 0 if nx is not a fourth power
int dim_q(int nx) {
  for (int d = 1; d * d * d * d <= nx; ++d)
    if (d * d * d * d == nx) return d;
  return 0;
}
// side of the plant operators: n (GENERATOR), d with d^4 = n (PROCESS), d with d^2 = n (HAMILTONIAN)
size_t plant_dim(int kind, int nx) {
  return kind == M4Q_PLANT_GENERATOR ? (size_t)nx : kind == M4Q_PLANT_PROCESS ? (size_t)dim_q(nx) : (size_t)dim_d(nx);
}

// An array that is per instance or shared, [B|1][elems]: the elements to allocate and the stride from one member's to the next
// (0: shared), from one expression - a size and a stride that disagree make a kernel read past its buffer.
struct Extent {
  size_t count;
  long stride;
  Extent(size_t B, bool per_instance, size_t elems) : count((per_instance ? B : 1) * elems), stride(per_instance ? (long)elems : 0) {}
};

int need_device() {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n == 0) return fail(M4Q_E_NODEVICE, "no HIP device: %s", hipGetErrorString(e));
  return 0;
}

int check_qp_flags(int32_t qp_flags) {
  if (qp_flags & ~(M4Q_QP_REF_LQR | M4Q_QP_DU_BAND | M4Q_QP_EXACT_BOX))
    return fail(M4Q_E_BADARG, "qp_flags has bits outside M4Q_QP_REF_LQR | M4Q_QP_DU_BAND | M4Q_QP_EXACT_BOX (0x%x)", qp_flags);
  if ((qp_flags & M4Q_QP_EXACT_BOX) && (qp_flags & M4Q_QP_REF_LQR))
    return fail(M4Q_E_BADARG, "M4Q_QP_EXACT_BOX cannot be combined with M4Q_QP_REF_LQR");
  return 0;
}

// one of the plants the one-shot entry points step on the device, and a process plant only on a state of d^4 entries.
// not_a_plant: the caller's message for any other kind (may print the kind with %d)
int check_device_plant_kind(int32_t kind, int32_t dim_x, const char* not_a_plant) {
  if (kind != M4Q_PLANT_HAMILTONIAN && kind != M4Q_PLANT_GENERATOR && kind != M4Q_PLANT_PROCESS) return fail(M4Q_E_BADARG, not_a_plant, kind);
  if (kind == M4Q_PLANT_PROCESS && dim_q(dim_x) == 0) return fail(M4Q_E_BADARG, "M4Q_PLANT_PROCESS: dim_x=%d is not a fourth power", dim_x);
  return 0;
}

// What the one-shot entry points on a plant refuse alike, before a device is asked for, in two parts with the entry's own argument
// checks in between.  named: the entry's name goes in front of the lookup's and of the process plant's refusal too (the entries
// from m4q_plant_quad_program_batch on; the earlier ones print those two bare).
//
// plant_shape: the object that holds the plant kernels of (dim_x, dim_u), plant-only ones included, and dim_x a square - every
// kernel behind these entries but plant_kernel's generator form has a density matrix or a process vector for a state.
// needs_qp: a plant-only object will not do either, it has no QP kernel.
int plant_shape(const char* who, bool named, int32_t dim_x, int32_t dim_u, bool needs_qp, const m4q::ShapeOps** found) {
  *found = find_shape_any_order(dim_x, dim_u, /*plant_ok=*/true);
  if (!*found) return fail(M4Q_E_UNSUPPORTED, "%s%sno kernel for dim_x=%d dim_u=%d", named ? who : "", named ? ": " : "", dim_x, dim_u);
  if (dim_d(dim_x) == 0) return fail(M4Q_E_UNSUPPORTED, "%s: dim_x=%d is not a square, there is no device plant", who, dim_x);
  if (needs_qp && (*found)->plant_only)
    return fail(M4Q_E_UNSUPPORTED, "%s: dim_x=%d dim_u=%d is a plant-only shape, it has no QP kernel", who, dim_x, dim_u);
  return 0;
}
// check_plant_kind: a device plant (check_device_plant_kind), and not the generator plant where the entry's kernels have no form
// for it - lacks names what is missing, advice what to call instead (lacks null: the generator plant is served)
int check_plant_kind(const char* who, bool named, int32_t kind, int32_t dim_x, const char* lacks, const char* advice) {
  if (int rc = check_device_plant_kind(kind, dim_x, (std::string(who) + ": plant_kind %d is not a device plant").c_str())) {
    if (named && kind == M4Q_PLANT_PROCESS) return fail(rc, "%s: M4Q_PLANT_PROCESS: dim_x=%d is not a fourth power", who, dim_x);
    return rc;
  }
  if (lacks && kind == M4Q_PLANT_GENERATOR)
    return fail(M4Q_E_UNSUPPORTED, "%s: the generator plant has no %s (its block matrix has (1 + m) n > 16 columns): %s", who, lacks, advice);
  return 0;
}

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  bool owned = true;
  int alloc(size_t n) {
    release();
    bytes = n;
    owned = true;
    if (n == 0) return 0;
    hipError_t e = hipMalloc(&p, n);
    if (e != hipSuccess) { p = nullptr; return fail(-(int)e, "hipMalloc(%zu): %s", n, hipGetErrorString(e)); }
    return 0;
  }
  void release() {
    if (p && owned) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  ~DevBuf() { release(); }
};

// The device side of one call: inputs uploaded, outputs allocated now and downloaded by finish(), everything freed with the
// object.  The first failure sticks: every later call is a no-op that returns null, so an entry point stages all its arrays,
// asks error() once before it launches and returns what finish() returns.
class Stage {
  struct Out { void* host; const void* dev; size_t bytes; };
  std::deque<DevBuf> bufs;
  std::vector<Out> outs;
  int rc = 0;
  void* device(size_t bytes) {
    if (rc) return nullptr;
    bufs.emplace_back();
    rc = bufs.back().alloc(bytes);
    return bufs.back().p;
  }

 public:
  int error() const { return rc; }
  // count elements of T copied to the device
  template <class T>
  const T* in(const void* host, size_t count) {
    void* d = device(count * sizeof(T));
    if (!rc && host && count) {
      hipError_t e = hipMemcpy(d, host, count * sizeof(T), hipMemcpyHostToDevice);
      if (e != hipSuccess) rc = fail(-(int)e, "hipMemcpy H2D: %s", hipGetErrorString(e));
    }
    return rc ? nullptr : static_cast<const T*>(d);
  }
  // count elements of T for the kernel to write; finish() copies them to host unless host is null (workspace)
  template <class T>
  T* out(void* host, size_t count) {
    void* d = device(count * sizeof(T));
    if (!rc && host && count) outs.push_back({host, d, count * sizeof(T)});
    return static_cast<T*>(d);
  }
  // after the launch on the null stream: its return code, the wait for the device, the downloads in the order of the out() calls
  int finish(int launch_rc, const char* what) {
    if (rc) return rc;
    if (launch_rc) return fail(launch_rc, "%s launch failed", what);
    HIP_TRY(hipDeviceSynchronize());
    for (const Out& o : outs) {
      hipError_t e = hipMemcpy(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost);
      if (e != hipSuccess) return fail(-(int)e, "hipMemcpy D2H: %s", hipGetErrorString(e));
    }
    return 0;
  }
};

// The operator block (m4q::PlantOps) over arrays that are on the device already, [B|1][k][k] and [B|1][m][k][k]: the strides
m4q::PlantOps plant_ops(const void* op0, const void* ops, size_t B, bool per_instance, size_t m, size_t k) {
  m4q::PlantOps p{};
  p.op0 = static_cast<const cplx*>(op0); p.op0_stride = Extent(B, per_instance, k * k).stride;
  p.ops = static_cast<const cplx*>(ops); p.ops_stride = Extent(B, per_instance, m * k * k).stride;
  return p;
}
// ... over the caller's arrays, staged: k from the plant kind, each size beside its stride
m4q::PlantOps stage_plant(Stage& st, int32_t B, int32_t kind, int32_t dim_x, int32_t dim_u, const double* op0, const double* ops,
                          int32_t plant_per_instance) {
  const size_t m = dim_u, k = plant_dim(kind, dim_x);
  const Extent e0(B, plant_per_instance, k * k), ek(B, plant_per_instance, m * k * k);
  m4q::PlantOps p{};
  p.op0 = st.in<cplx>(op0, e0.count); p.op0_stride = e0.stride;
  p.ops = st.in<cplx>(ops, ek.count); p.ops_stride = ek.stride;
  return p;
}
// ... with the trajectories of B members over T points a linearisation runs along (m4q::PlantTraj)
m4q::PlantTraj stage_traj(Stage& st, int32_t B, int32_t kind, int32_t dim_x, int32_t dim_u, int32_t T, const double* dts, const double* X,
                          const double* U, int32_t u_per_instance, const double* u_scale, const double* op0, const double* ops,
                          int32_t plant_per_instance) {
  const size_t n = dim_x, m = dim_u;
  const Extent eu(B, u_per_instance, (size_t)T * m);
  m4q::PlantTraj t{};
  t.dts = st.in<double>(dts, T);
  t.X = st.in<cplx>(X, (size_t)B * T * n);
  t.U = st.in<double>(U, eu.count); t.u_stride = eu.stride;
  if (u_scale) t.u_scale = st.in<double>(u_scale, (size_t)B * m);
  t.plant = stage_plant(st, B, kind, dim_x, dim_u, op0, ops, plant_per_instance);
  return t;
}

// symmetrised real-ified cost block of iqp_line_search (mpc.py:92-93,103-104,112-116)
void ls_block(const double* M, int k, std::vector<double>& out) {
  const int s = 2 * k;
  std::vector<double> c((size_t)s * s);
  for (int i = 0; i < k; ++i)
    for (int j = 0; j < k; ++j) {
      const double re = M[2 * (i * k + j)], im = M[2 * (i * k + j) + 1];
      c[(size_t)i * s + j] = re;
      c[(size_t)i * s + (j + k)] = -im;
      c[(size_t)(i + k) * s + j] = im;
      c[(size_t)(i + k) * s + (j + k)] = re;
    }
  out.resize((size_t)s * s);
  for (int i = 0; i < s; ++i)
    for (int j = 0; j < s; ++j) out[(size_t)i * s + j] = 0.5 * (c[(size_t)i * s + j] + c[(size_t)j * s + i]);
}

}  // namespace

struct m4q_session {
  m4q_problem prob{};
  int B = 0;
  int device = 0;
  const m4q::ShapeOps* shape = nullptr;
  const m4q::ShapeOps* mpc_ops = nullptr;      // launch_mpc / occupancy / mpc_lds_bytes: `shape`, or libm4q_hip_gen.so's for the generator plant
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool allowed[m4q::PATH_SG + 1] = {};   // [m4q::Path]: the paths the shape, the options and the problem admit (m4q_session_create)
  int grid = 1;                 // resident workgroups of the launch (PATH_COMPLEX .. PATH_TILE); the per-row workspace is sized for max(grid, grid_sg)
  int grid_sg = 0;              // ... of the shared-generator kernel (PATH_SG: two wavefronts per SIMD at d = 4)
  // shared-generator form (m4q_session_build_models with ONE generator set, order 1, traceless blocks): dt L_k on the traceless
  // coordinates [1 + m][n-1][n-1] and the members' scales [B][1 + m]; the kernel of PATH_SG reads these instead of the models
  DevBuf sg_gens, sg_scales;
  bool sg_ok = false;
  DevBuf f[M4Q_F_COUNT];
  DevBuf Cq, Cqf, Cr, Wls, wsXg, wsUg, wsG, queue, head_done;
  size_t fbytes[M4Q_F_COUNT]{};
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;   // (start, stop) of launches not yet read by kernel_ms
  double folded_ms = 0.0;                                    // launches already completed and folded out of `pending`
  int folded_n = 0;
  double ms_total = 0.0;
  int launches = 0;
  bool costs_dirty = true;
  bool ls_diag = false;
  // the inputs the recursion reads, on the real coordinate systems ([COORDS_HERM], [COORDS_TRACELESS]; the complex copy is f[]):
  // lifted at upload time, and whether each qualified there (Lift).  tau_*: the range of trace coordinates seen in x0 / X_targ
  // (state and target must share ONE trace for the cost to restrict to the traceless coordinates)
  struct Copy { DevBuf buf; bool ok = false; };
  Copy copies[m4q::COORDS_TRACELESS + 1][M4Q_F_COUNT];
  double tau_x0[2] = {0, 0}, tau_targ[2] = {0, 0};
  bool launched = false;        // a closed-loop launch has been enqueued since the watchdog flag was last read
  bool targ_const = false;      // every column of X_targ equals the first (per member, if per-member): xbar does not depend on t
  // exit condition (m4q_session_set_exit): M4Q_EXIT_* bits (0: none), W [n][n] c, target [B|1][n] c, thresholds [B|1]
  int exit_mode = 0;
  bool exit_target_per = false, exit_thr_per = false;
  DevBuf exit_W, exit_target, exit_thr;
  // measurement noise (m4q_session_set_noise): M4Q_NOISE_* (0: none), sigma [B|1], the generator's seed, the global index of member 0
  int noise_mode = 0;
  bool noise_sigma_per = false;
  DevBuf noise_sigma;
  uint64_t noise_seed = 0, noise_member_base = 0;
  bool ran = false;             // m4q_session_run has been called: the noise mode is fixed from here on
  // observed plant (m4q_session_set_observed_plant; PLANT_NONE sessions): M4Q_OBSERVE_* (0: none), the plant's operators
  // [B|1][d_p][d_p] and [B|1][m][d_p][d_p], its states zs [B][n_steps + 1][n_p], the shape whose object holds the kernels
  int observe = 0;
  bool obs_per = false;
  DevBuf obs_op0, obs_ops, zs;
  const m4q::ShapeOps* obs_shape = nullptr;
  std::vector<double> hQ, hQf, hR;

  // R weighs the controls, which are real on every path: its one real copy ([COORDS_HERM]) serves both real coordinate systems
  const Copy& copy(int field, m4q::Coords c) const { return copies[field == M4Q_F_R ? m4q::COORDS_HERM : c][field]; }
  // the device array of input `field` on coordinates c
  const void* input(int field, m4q::Coords c) const { return c == m4q::COORDS_COMPLEX ? f[field].p : copy(field, c).buf.p; }
  bool qualified(m4q::Coords c) const {
    for (int field : {M4Q_F_MODELS, M4Q_F_X0, M4Q_F_X_TARG, M4Q_F_Q, M4Q_F_QF, M4Q_F_R})
      if (!copy(field, c).ok) return false;
    return true;
  }
  // the first allowed path the uploaded data support.  diag: the line-search blocks of the costs are diagonal (known after the first
  // run; m4q_session_path answers as if they were before that)
  m4q::Path path(bool diag) const {
    if (noise_mode == M4Q_NOISE_IID) return m4q::PATH_COMPLEX;      // independent noise on every component: the state is not Hermitian
    const double lo = std::min(tau_x0[0], tau_targ[0]), hi = std::max(tau_x0[1], tau_targ[1]);
    const bool real = diag && qualified(m4q::COORDS_HERM);
    const bool traceless = real && qualified(m4q::COORDS_TRACELESS) && hi - lo <= 1e-12 * std::max(1.0, std::fabs(hi));
    const bool supported[m4q::PATH_SG + 1] = {true, real, traceless, traceless && targ_const, traceless && sg_ok};
    for (m4q::Path p : {m4q::PATH_SG, m4q::PATH_TILE, m4q::PATH_TRACELESS, m4q::PATH_REAL})
      if (allowed[p] && supported[p]) return p;
    return m4q::PATH_COMPLEX;
  }
  m4q::Path path() const { return path(ls_diag); }
};

extern "C" {

const char* m4q_last_error(void) { return g_err.c_str(); }
const char* m4q_version(void) { return "m4q-hip 0.1 (gfx950)"; }

int m4q_device_count(void) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) return fail(-(int)e, "hipGetDeviceCount: %s", hipGetErrorString(e));
  return n;
}

int m4q_supported(int32_t dim_x, int32_t dim_u, int32_t order) { return find_shape(dim_x, dim_u, order) ? 1 : 0; }

int m4q_library_size(int32_t order, int32_t dim_u) {
  if (order < 0 || dim_u < 1) return fail(M4Q_E_BADARG, "bad (order, dim_u)");
  // C(order + m, m) - 1
  long r = 1;
  for (int i = 1; i <= dim_u; ++i) r = r * (order + i) / i;
  return (int)r - 1;
}

int m4q_power_list(int32_t order, int32_t dim_u, int32_t* out) {
  for (int nx : {4, 9, 16})
    if (const m4q::ShapeOps* s = find_shape(nx, dim_u, order)) return s->power_list(out);
  return fail(M4Q_E_UNSUPPORTED, "no compiled kernel with (order=%d, dim_u=%d)", order, dim_u);
}

// ------------------------------------------------------------------------------------------
// session
// ------------------------------------------------------------------------------------------
int m4q_session_create(const m4q_problem* p, int32_t B, int32_t device, m4q_session** out) {
  if (!p || !out || B <= 0) return fail(M4Q_E_BADARG, "m4q_session_create: bad argument");
  const m4q::ShapeOps* sh = find_shape(p->dim_x, p->dim_u, p->order);
  if (!sh) return fail(M4Q_E_UNSUPPORTED, "no kernel for dim_x=%d dim_u=%d order=%d", p->dim_x, p->dim_u, p->order);
  if (p->horizon < 1 || p->n_steps < 1 || p->target_cols < p->horizon + 1 + (p->n_steps > 1 ? p->n_steps - 2 : 0))
    return fail(M4Q_E_BADARG, "horizon/n_steps/target_cols inconsistent (need target_cols >= n_steps + horizon - 1)");
  if (!(p->sat > 0)) return fail(M4Q_E_BADARG, "sat must be positive (the reference crashes on sat=None, mpc.py Q5)");
  if (int rc = check_qp_flags(p->qp_flags)) return rc;
  if (p->plant_kind == M4Q_PLANT_PROCESS && dim_q(p->dim_x) == 0)
    return fail(M4Q_E_BADARG, "M4Q_PLANT_PROCESS: dim_x=%d is not a fourth power (the process vector of a d x d unitary has d^4 entries)",
                p->dim_x);
  {
    // per-instance targets / plant operators are reached through 32-bit byte offsets from one base
    const double lim = 4294967296.0;
    const double kk = (double)plant_dim(p->plant_kind, p->dim_x);
    if (p->target_per_instance && (double)B * p->target_cols * p->dim_x * 16.0 >= lim)
      return fail(M4Q_E_BADARG, "per-instance targets must stay below 4 GiB in total");
    if (p->plant_per_instance && (double)B * p->dim_u * kk * kk * 16.0 >= lim)
      return fail(M4Q_E_BADARG, "per-instance plant operators must stay below 4 GiB in total");
  }
  if (int rc = need_device()) return rc;
  if (device >= 0) HIP_TRY(hipSetDevice(device));
  m4q_session* s = new m4q_session();
  s->prob = *p;
  s->B = B;
  s->shape = sh;
  s->mpc_ops = sh;
  if (p->plant_kind == M4Q_PLANT_GENERATOR) {
    std::string why;
    s->mpc_ops = gen_shape(p->dim_x, p->dim_u, p->order, why);
    if (!s->mpc_ops) {
      delete s;
      return fail(M4Q_E_UNSUPPORTED, "%s", why.c_str());
    }
  }
  if (sh->d * sh->d != p->dim_x && p->plant_kind != M4Q_PLANT_NONE) {
    delete s;
    return fail(M4Q_E_UNSUPPORTED, "dim_x=%d is not a vectorised density matrix: no device plant (use M4Q_PLANT_NONE)", p->dim_x);
  }
  HIP_TRY_OWNED(s, hipGetDevice(&s->device));
  HIP_TRY_OWNED(s, hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
  HIP_TRY_OWNED(s, hipEventCreate(&s->ev0));
  HIP_TRY_OWNED(s, hipEventCreate(&s->ev1));
  const size_t n = p->dim_x, m = p->dim_u, P = sh->np, T = p->horizon, ns = p->n_steps, cols = p->target_cols;
  const size_t k = plant_dim(p->plant_kind, p->dim_x);
  const size_t C = 16;
  const bool has_plant = p->plant_kind != M4Q_PLANT_NONE;
  size_t* fb = s->fbytes;
  fb[M4Q_F_MODELS] = Extent(B, p->model_per_instance, n * n * (1 + P)).count * C;
  fb[M4Q_F_X0] = (size_t)B * n * C;
  fb[M4Q_F_X_TARG] = Extent(B, p->target_per_instance, cols * n).count * C;
  fb[M4Q_F_U_TARG] = Extent(B, p->target_per_instance, cols * m).count * 8;
  fb[M4Q_F_Q] = n * n * C;
  fb[M4Q_F_QF] = n * n * C;
  fb[M4Q_F_R] = m * m * C;
  fb[M4Q_F_OP0] = has_plant ? Extent(B, p->plant_per_instance, k * k).count * C : 0;
  fb[M4Q_F_OPS] = has_plant ? Extent(B, p->plant_per_instance, m * k * k).count * C : 0;
  fb[M4Q_F_XS] = (size_t)B * (ns + 1) * n * C;
  fb[M4Q_F_US] = (size_t)B * ns * m * 8;
  fb[M4Q_F_CODES] = (size_t)B * 4;
  fb[M4Q_F_STEPS_DONE] = (size_t)B * 4;
  fb[M4Q_F_QP_SOLVES] = (size_t)B * ns * 4;
  fb[M4Q_F_X_GUESS] = (size_t)B * (T + 1) * n * C;
  fb[M4Q_F_U_GUESS] = (size_t)B * T * m * 8;
  int rc = 0;
  for (int i = 0; i < M4Q_F_COUNT && !rc; ++i) rc = s->f[i].alloc(fb[i]);
  // The paths this session may take; the uploaded data choose among them (m4q_session::path).  A process plant runs on the complex
  // path alone: V (x) V^* does not keep M Hermitian as a d^2 x d^2 matrix, so the Hermitian lift of data that happens to pass it
  // would still be wrong after the first plant step.  M4Q_QP_REF_LQR builds its cost terms on xbar itself (lqr.py:54-58): the trace
  // coordinate of the target does not drop out.  The tile form of the sweeps is what a traceless session with a constant target runs
  // wherever it is built (d = 2, 3 with an order-1 library: include/m4q.h, M4Q_OPT_NO_TILE).
  const int exact = (p->qp_flags & M4Q_QP_EXACT_BOX) ? 1 : 0;
  bool* allow = s->allowed;
  allow[m4q::PATH_COMPLEX] = true;
  allow[m4q::PATH_REAL] = !(p->reserved & M4Q_OPT_FORCE_COMPLEX) && !std::getenv("M4Q_FORCE_COMPLEX") && sh->d * sh->d == p->dim_x &&
                          p->plant_kind != M4Q_PLANT_PROCESS;
  allow[m4q::PATH_TRACELESS] = allow[m4q::PATH_REAL] && !(p->reserved & M4Q_OPT_NO_TRACELESS) && !std::getenv("M4Q_NO_TRACELESS") &&
                               !(p->qp_flags & M4Q_QP_REF_LQR);
  allow[m4q::PATH_TILE] = allow[m4q::PATH_TRACELESS] && sh->has_tile && !(p->reserved & M4Q_OPT_NO_TILE) && !std::getenv("M4Q_NO_TILE");
  allow[m4q::PATH_SG] = allow[m4q::PATH_TRACELESS] && sh->has_sg && !(p->reserved & M4Q_OPT_NO_SG) && !std::getenv("M4Q_NO_SG") &&
                        !exact && p->order == 1;
  // resident grid: as many workgroups as the device holds at once (persistent, quad-strided), sized for whichever allowed path keeps
  // more of them resident; the shared-generator kernel keeps more than the per-member-model kernels of its shape: its own grid
  hipDeviceProp_t prop;
  HIP_TRY_OWNED(s, hipGetDeviceProperties(&prop, s->device));
  const char* cap = std::getenv("M4Q_WGS_PER_CU");            // tuning experiments: fewer resident workgroups per CU
  const int cap_v = cap ? std::atoi(cap) : 0;
  const long nquads = (B + 3) / 4;
  auto resident = [&](int per_cu) {
    if (cap_v >= 1 && cap_v < per_cu) per_cu = cap_v;
    return (int)std::min(nquads, (long)per_cu * prop.multiProcessorCount);
  };
  const m4q::ShapeOps* mo = s->mpc_ops;
  int per_cu = 1;
  for (m4q::Path q : {m4q::PATH_COMPLEX, m4q::PATH_REAL, m4q::PATH_TRACELESS, m4q::PATH_TILE})
    if (allow[q]) per_cu = std::max(per_cu, mo->occupancy(p->plant_kind, q, exact));
  s->grid = resident(per_cu);
  if (allow[m4q::PATH_SG]) {
    const int pc = mo->occupancy(p->plant_kind, m4q::PATH_SG, exact);
    if (pc >= 1) s->grid_sg = resident(pc);
    else allow[m4q::PATH_SG] = false;
  }
  const size_t rows = (size_t)std::max(s->grid, s->grid_sg) * 4;
  // [Xg rows][Xo rows] and [Ug rows][Uo rows]; the exact QP adds [Xalt rows] and [Ualt rows][working-set rows]
  if (!rc) rc = s->wsXg.alloc((exact ? 3 : 2) * rows * (T + 1) * n * C);
  if (!rc) rc = s->wsUg.alloc((exact ? 4 : 2) * rows * T * m * 8);
  if (!rc) rc = s->queue.alloc(192);       // 64 B of queue / watchdog / solver counters + 16 u64 phase clocks (dev builds)
  if (!rc) rc = s->head_done.alloc((size_t)B * 4);
  if (!rc) rc = s->wsG.alloc(rows * T * (n + 1) * m * C);
  if (!rc) rc = s->Cq.alloc(4 * n * n * 8);
  if (!rc) rc = s->Cqf.alloc(4 * n * n * 8);
  if (!rc) rc = s->Cr.alloc(4 * m * m * 8);
  if (!rc) rc = s->Wls.alloc((4 * n + 2 * m) * 8);
  if (rc) { m4q_session_destroy(s); return rc; }
  for (int i : {M4Q_F_XS, M4Q_F_US, M4Q_F_CODES, M4Q_F_STEPS_DONE, M4Q_F_QP_SOLVES})
    HIP_TRY_OWNED(s, hipMemsetAsync(s->f[i].p, 0, fb[i], s->stream));
  HIP_TRY_OWNED(s, hipStreamSynchronize(s->stream));
  *out = s;
  return 0;
}

void m4q_session_destroy(m4q_session* s) {
  if (!s) return;
  for (auto& pr : s->pending) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
  if (s->ev0) (void)hipEventDestroy(s->ev0);
  if (s->ev1) (void)hipEventDestroy(s->ev1);
  if (s->stream) (void)hipStreamDestroy(s->stream);
  delete s;
}

size_t m4q_session_field_bytes(const m4q_session* s, int32_t field) {
  if (!s || field < 0 || field >= M4Q_F_COUNT) return 0;
  return s->fbytes[field];
}

// After the stream has drained: did the last closed-loop launch leave through its watchdog?
static int check_watchdog(m4q_session* s) {
  if (!s->launched) return 0;
  s->launched = false;
  int flag = 0;
  HIP_TRY(hipMemcpy(&flag, (const char*)s->queue.p + 4, 4, hipMemcpyDeviceToHost));
  if (flag) HIP_TRY(hipMemset((char*)s->queue.p + 4, 0, 4));
  if (flag)
    return fail(M4Q_E_TIMEOUT, "the closed-loop kernel abandoned the launch: its watchdog expired (M4Q_KERNEL_TIMEOUT_S, default 300 s "
                               "of device time) before every ensemble member had finished; this launch's results are not valid");
  return 0;
}

int m4q_session_upload(m4q_session* s, int32_t field, const void* host, size_t bytes) {
  if (!s || field < 0 || field >= M4Q_F_COUNT || !host) return fail(M4Q_E_BADARG, "m4q_session_upload: bad argument");
  if (bytes != s->fbytes[field]) return fail(M4Q_E_BADARG, "field %d expects %zu bytes, got %zu", field, s->fbytes[field], bytes);
  if (bytes == 0) return 0;
  HIP_TRY(hipMemcpyAsync(s->f[field].p, host, bytes, hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  const size_t n = s->prob.dim_x, m = s->prob.dim_u, P = s->shape->np;
  const auto* ch = static_cast<const std::complex<double>*>(host);
  if (field == M4Q_F_Q) { s->hQ.assign((const double*)host, (const double*)host + 2 * n * n); s->costs_dirty = true; }
  if (field == M4Q_F_QF) { s->hQf.assign((const double*)host, (const double*)host + 2 * n * n); s->costs_dirty = true; }
  if (field == M4Q_F_R) { s->hR.assign((const double*)host, (const double*)host + 2 * m * m); s->costs_dirty = true; }
  if (field == M4Q_F_X_TARG) {
    const size_t cols = s->prob.target_cols, items = bytes / (16 * n * cols);
    bool same = true;
    for (size_t it = 0; it < items && same; ++it)
      for (size_t c = 1; c < cols && same; ++c)
        same = std::memcmp(ch + (it * cols + c) * n, ch + it * cols * n, 16 * n) == 0;
    s->targ_const = same;
  }
  if (!s->allowed[m4q::PATH_REAL]) return 0;
  // the inputs the recursion reads, on the real coordinate systems
  const int d = s->shape->d;
  const bool tl = s->allowed[m4q::PATH_TRACELESS];
  Lift L;
  switch (field) {
    case M4Q_F_MODELS:
      s->sg_ok = false;                         // uploaded models: not (known to be) an ensemble of scaled shared generators
      L = lift_blocks(d, ch, bytes / (16 * n * n * (1 + P)), (int)(1 + P), true, tl);
      break;
    case M4Q_F_X0:
    case M4Q_F_X_TARG:
      L = lift_vectors(d, ch, bytes / (16 * n), tl);
      std::copy(L.tau, L.tau + 2, field == M4Q_F_X0 ? s->tau_x0 : s->tau_targ);
      break;
    case M4Q_F_Q:
    case M4Q_F_QF:
      // the cross terms with the (constant, shared) trace coordinate drop out of the objective's minimiser: nothing to check
      L = lift_blocks(d, ch, 1, 1, false, tl);
      L.ok[m4q::COORDS_TRACELESS] = !L.v[m4q::COORDS_TRACELESS].empty();
      break;
    case M4Q_F_R: {
      // R acts on the (real) controls: its real part, and the real paths need Im R = 0
      LiftStat st;
      L.v[m4q::COORDS_HERM].resize(m * m);
      for (size_t i = 0; i < m * m; ++i) { st.see(ch[i]); L.v[m4q::COORDS_HERM][i] = ch[i].real(); }
      L.ok[m4q::COORDS_HERM] = st.real_enough();
      break;
    }
    default:
      return 0;
  }
  for (m4q::Coords c : {m4q::COORDS_HERM, m4q::COORDS_TRACELESS}) {
    m4q_session::Copy& dst = s->copies[c][field];
    dst.ok = false;
    if (L.v[c].empty()) continue;
    if (int rc = dst.buf.alloc(L.v[c].size() * 8)) return rc;
    HIP_TRY(hipMemcpy(dst.buf.p, L.v[c].data(), L.v[c].size() * 8, hipMemcpyHostToDevice));
    dst.ok = L.ok[c];
  }
  return 0;
}

int m4q_session_path(const m4q_session* s) {
  if (!s) return fail(M4Q_E_BADARG, "m4q_session_path: null session");
  // the line-search weights are derived from Q, Qf, R at the first run; before that, answer from the uploads alone
  const bool diag_known = !s->costs_dirty;
  return s->path(diag_known ? s->ls_diag : true);
}

int m4q_session_download(m4q_session* s, int32_t field, void* host, size_t bytes) {
  if (!s || field < 0 || field >= M4Q_F_COUNT || !host) return fail(M4Q_E_BADARG, "m4q_session_download: bad argument");
  if (bytes != s->fbytes[field]) return fail(M4Q_E_BADARG, "field %d holds %zu bytes, asked %zu", field, s->fbytes[field], bytes);
  if (bytes == 0) return 0;
  HIP_TRY(hipMemcpyAsync(host, s->f[field].p, bytes, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return check_watchdog(s);
}

int m4q_session_put_state(m4q_session* s, int32_t step, const void* host) {
  if (!s || !host || step < 0 || step > s->prob.n_steps) return fail(M4Q_E_BADARG, "m4q_session_put_state: bad argument");
  const size_t row = (size_t)s->prob.dim_x * 16;
  HIP_TRY(hipMemcpy2DAsync((char*)s->f[M4Q_F_XS].p + (size_t)step * row, (size_t)(s->prob.n_steps + 1) * row, host, row, row,
                           s->B, hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return check_watchdog(s);
}

int m4q_session_get_state(m4q_session* s, int32_t step, void* host) {
  if (!s || !host || step < 0 || step > s->prob.n_steps) return fail(M4Q_E_BADARG, "m4q_session_get_state: bad argument");
  const size_t row = (size_t)s->prob.dim_x * 16;
  HIP_TRY(hipMemcpy2DAsync(host, row, (const char*)s->f[M4Q_F_XS].p + (size_t)step * row, (size_t)(s->prob.n_steps + 1) * row,
                           row, s->B, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return check_watchdog(s);
}

void* m4q_session_device_ptr(m4q_session* s, int32_t field) {
  if (!s || field < 0 || field >= M4Q_F_COUNT) return nullptr;
  return s->f[field].p;
}

int m4q_session_bind_output(m4q_session* s, int32_t field, void* device_ptr, size_t bytes) {
  if (!s || !device_ptr || field < M4Q_F_XS || field >= M4Q_F_COUNT) return fail(M4Q_E_BADARG, "m4q_session_bind_output: bad field");
  if (bytes != s->fbytes[field]) return fail(M4Q_E_BADARG, "field %d expects %zu bytes, got %zu", field, s->fbytes[field], bytes);
  s->f[field].release();
  s->f[field].p = device_ptr;
  s->f[field].bytes = bytes;
  s->f[field].owned = false;
  return 0;
}

static int refresh_costs(m4q_session* s) {
  if (!s->costs_dirty) return 0;
  const int n = s->prob.dim_x, m = s->prob.dim_u;
  if (s->hQ.empty() || s->hQf.empty() || s->hR.empty()) return fail(M4Q_E_BADARG, "Q, Qf and R must be uploaded before running");
  std::vector<double> c, w;
  bool diag = true;
  auto take_diag = [&](int k) {
    const int sz = 2 * k;
    for (int i = 0; i < sz; ++i)
      for (int j2 = 0; j2 < sz; ++j2)
        if (i != j2 && c[(size_t)i * sz + j2] != 0.0) diag = false;
    for (int i = 0; i < sz; ++i) w.push_back(c[(size_t)i * sz + i]);
  };
  ls_block(s->hQ.data(), n, c);
  HIP_TRY(hipMemcpy(s->Cq.p, c.data(), c.size() * 8, hipMemcpyHostToDevice));
  take_diag(n);
  ls_block(s->hQf.data(), n, c);
  HIP_TRY(hipMemcpy(s->Cqf.p, c.data(), c.size() * 8, hipMemcpyHostToDevice));
  take_diag(n);
  ls_block(s->hR.data(), m, c);
  HIP_TRY(hipMemcpy(s->Cr.p, c.data(), c.size() * 8, hipMemcpyHostToDevice));
  take_diag(m);
  HIP_TRY(hipMemcpy(s->Wls.p, w.data(), w.size() * 8, hipMemcpyHostToDevice));
  s->ls_diag = diag;
  s->costs_dirty = false;
  return 0;
}

int m4q_session_run(m4q_session* s, int32_t step_begin, int32_t step_end) {
  if (!s || step_begin < 0 || step_end > s->prob.n_steps || step_begin >= step_end)
    return fail(M4Q_E_BADARG, "m4q_session_run: bad step range [%d, %d)", step_begin, step_end);
  int rc = refresh_costs(s);
  if (rc) return rc;
  const m4q_problem& p = s->prob;
  const size_t n = p.dim_x, m = p.dim_u, P = s->shape->np;
  const size_t k = plant_dim(p.plant_kind, p.dim_x);
  const m4q::Path path = s->path();
  const m4q::Coords coords = m4q::coords_of(path);
  const size_t ns = coords == m4q::COORDS_TRACELESS ? n - 1 : n;         // dimension of the recursion
  m4q::MpcArgs a{};
  a.B = s->B; a.T = p.horizon; a.n_steps = p.n_steps; a.max_iter = p.max_iter; a.warm_start = p.warm_start;
  a.flags = p.qp_flags | (s->targ_const ? m4q::QP_TARG_CONST : 0) | (s->allowed[m4q::PATH_TILE] ? 0 : m4q::QP_NO_TILE);
  a.step_begin = step_begin; a.step_end = step_end;
  a.measure_freq = p.measure_freq > 1 ? p.measure_freq : 1;
  a.dt = p.dt; a.sat = p.sat; a.du = p.du; a.ls_tol = p.ls_tol;
  a.models = s->input(M4Q_F_MODELS, coords);
  a.gens = (const double*)s->sg_gens.p; a.scales = (const double*)s->sg_scales.p;
  a.exit_mode = s->exit_mode;
  a.exit_W = (const cplx*)s->exit_W.p;
  a.exit_target = (const cplx*)s->exit_target.p; a.exit_tstride = Extent(s->B, s->exit_target_per, n).stride;
  a.exit_thr = (const double*)s->exit_thr.p; a.exit_thr_stride = Extent(s->B, s->exit_thr_per, 1).stride;
  a.noise_mode = s->noise_mode;
  a.noise_sigma = (const double*)s->noise_sigma.p; a.noise_sigma_stride = Extent(s->B, s->noise_sigma_per, 1).stride;
  a.noise_seed = s->noise_seed; a.noise_member_base = s->noise_member_base;
  a.model_stride = Extent(s->B, p.model_per_instance, ns * ns * (1 + P)).stride;
  a.x0c = (const cplx*)s->f[M4Q_F_X0].p;
  a.x0s = s->input(M4Q_F_X0, coords);
  a.x_targ = s->input(M4Q_F_X_TARG, coords);
  a.xt_stride = Extent(s->B, p.target_per_instance, p.target_cols * ns).stride;
  a.u_targ = (const double*)s->f[M4Q_F_U_TARG].p; a.ut_stride = Extent(s->B, p.target_per_instance, p.target_cols * m).stride;
  a.Q = s->input(M4Q_F_Q, coords); a.Qf = s->input(M4Q_F_QF, coords); a.R = s->input(M4Q_F_R, coords);
  a.Cq = (const double*)s->Cq.p; a.Cqf = (const double*)s->Cqf.p; a.Cr = (const double*)s->Cr.p;
  a.Wls = s->ls_diag ? (const double*)s->Wls.p : nullptr;
  a.plant = plant_ops(s->f[M4Q_F_OP0].p, s->f[M4Q_F_OPS].p, s->B, p.plant_per_instance, m, k);
  if (p.plant_kind == M4Q_PLANT_NONE) a.plant = plant_ops(s->f[M4Q_F_Q].p, s->f[M4Q_F_Q].p, s->B, false, m, k);
  a.xs = (cplx*)s->f[M4Q_F_XS].p; a.us = (double*)s->f[M4Q_F_US].p;
  a.codes = (int*)s->f[M4Q_F_CODES].p; a.steps_done = (int*)s->f[M4Q_F_STEPS_DONE].p; a.qp_solves = (int*)s->f[M4Q_F_QP_SOLVES].p;
  a.Xg = (cplx*)s->f[M4Q_F_X_GUESS].p; a.Ug = (double*)s->f[M4Q_F_U_GUESS].p;
  a.ws_Xg = s->wsXg.p; a.ws_Ug = (double*)s->wsUg.p;
  a.ws_gains = s->wsG.p;
  a.queue = (int*)s->queue.p;
  a.head_done = (int*)s->head_done.p;
  {
    double seconds = 300.0;                                  // below the 7 minutes of silence after which a GPU box kills a job
    if (const char* e = std::getenv("M4Q_KERNEL_TIMEOUT_S")) {
      const double v = std::atof(e);
      if (v > 0) seconds = v;
    }
    a.deadline_ticks = (unsigned long long)(seconds * 1e8);  // s_memrealtime counts at 100 MHz
  }
  if (s->launched) {
    // an earlier launch has not been synchronised yet: its watchdog flag (bytes 4..8) must survive until check_watchdog reads it
    HIP_TRY(hipMemsetAsync(s->queue.p, 0, 4, s->stream));
    HIP_TRY(hipMemsetAsync((char*)s->queue.p + 8, 0, 184, s->stream));
  } else {
    HIP_TRY(hipMemsetAsync(s->queue.p, 0, 192, s->stream));
  }
  HIP_TRY(hipMemsetAsync(s->head_done.p, 0, (size_t)s->B * 4, s->stream));
  if (step_begin == 0) {
    HIP_TRY(hipMemsetAsync(s->f[M4Q_F_QP_SOLVES].p, 0, s->fbytes[M4Q_F_QP_SOLVES], s->stream));
    HIP_TRY(hipMemsetAsync(s->f[M4Q_F_CODES].p, 0, s->fbytes[M4Q_F_CODES], s->stream));
    HIP_TRY(hipMemsetAsync(s->f[M4Q_F_STEPS_DONE].p, 0, s->fbytes[M4Q_F_STEPS_DONE], s->stream));
  }
  // a long step-by-step run never reads its timings: fold finished launches so the event list stays short
  while (s->pending.size() > 64 && hipEventQuery(s->pending.front().second) == hipSuccess) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, s->pending.front().first, s->pending.front().second) == hipSuccess) {
      s->folded_ms += ms;
      ++s->folded_n;
    }
    (void)hipEventDestroy(s->pending.front().first);
    (void)hipEventDestroy(s->pending.front().second);
    s->pending.erase(s->pending.begin());
  }
  hipEvent_t e0, e1;
  HIP_TRY(hipEventCreate(&e0));
  HIP_TRY(hipEventCreate(&e1));
  HIP_TRY(hipEventRecord(e0, s->stream));
  rc = s->mpc_ops->launch_mpc(a, p.plant_kind, path, path == m4q::PATH_SG ? s->grid_sg : s->grid, s->stream);
  if (rc) return fail(rc, "mpc kernel launch failed: %s", hipGetErrorString((hipError_t)(-rc)));
  HIP_TRY(hipEventRecord(e1, s->stream));
  s->pending.emplace_back(e0, e1);
  s->launched = true;
  s->ran = true;
  return 0;
}

// ------------------------------------------------------------------------------------------
// observed plants (m4q_observe.h)
// ------------------------------------------------------------------------------------------
static int check_observe_kind(const char* who, int32_t observe) {
  if (observe != M4Q_OBSERVE_PARTIAL_TRACE && observe != M4Q_OBSERVE_QUBIT_BLOCK)
    return fail(M4Q_E_BADARG, "%s: observe %d is not M4Q_OBSERVE_PARTIAL_TRACE or M4Q_OBSERVE_QUBIT_BLOCK", who, observe);
  return 0;
}

int m4q_observe_batch(int32_t B, int32_t observe, const double* z, double* x) {
  if (B < 1 || !z || !x) return fail(M4Q_E_BADARG, "m4q_observe_batch: bad argument (B >= 1, z, x)");
  if (int rc = check_observe_kind("m4q_observe_batch", observe)) return rc;
  const int n = m4q::observe_n(observe), np = m4q::observe_np(observe);
  const m4q::ShapeOps* sh = nullptr;
  for (int nu = 1; nu <= 3 && !sh; ++nu) sh = find_shape_any_order(n, nu);
  if (!sh || sh->observe_kind != observe) return fail(M4Q_E_UNSUPPORTED, "m4q_observe_batch: no compiled kernel with dim_x=%d", n);
  if (int rc = need_device()) return rc;
  Stage st;
  m4q::ObserveArgs a{};
  a.B = B; a.kind = observe;
  a.z = st.in<cplx>(z, (size_t)B * np); a.z_stride = np;
  a.x = st.out<cplx>(x, (size_t)B * n); a.x_stride = n;
  if (st.error()) return st.error();
  return st.finish(sh->launch_observe(a, nullptr), "observe kernel");
}

int m4q_session_set_observed_plant(m4q_session* s, int32_t observe, const double* op0, const double* ops, int32_t plant_per_instance,
                                   const double* z0) {
  if (!s || !op0 || !ops || !z0) return fail(M4Q_E_BADARG, "m4q_session_set_observed_plant: bad argument (session, op0, ops, z0)");
  if (int rc = check_observe_kind("m4q_session_set_observed_plant", observe)) return rc;
  const m4q_problem& p = s->prob;
  if (p.plant_kind != M4Q_PLANT_NONE)
    return fail(M4Q_E_BADARG, "m4q_session_set_observed_plant: the session has a device plant (plant_kind %d); an observed plant is a "
                "setting of an M4Q_PLANT_NONE session", p.plant_kind);
  if (p.measure_freq > 1)
    return fail(M4Q_E_BADARG, "m4q_session_set_observed_plant: measure_freq = %d; an observed plant is measured at every step",
                p.measure_freq);
  if (p.dim_x != m4q::observe_n(observe))
    return fail(M4Q_E_BADARG, "m4q_session_set_observed_plant: observe %d gives loop states of %d entries, the session has dim_x = %d",
                observe, m4q::observe_n(observe), p.dim_x);
  if (s->ran)
    return fail(M4Q_E_BADARG, "m4q_session_set_observed_plant: the session has already run; the plant is set before the first run");
  const size_t B = s->B, m = p.dim_u, ns = p.n_steps, n = p.dim_x, C = 16;
  const size_t np = m4q::observe_np(observe), dp = m4q::observe_dp(observe);
  if (plant_per_instance && (double)B * m * dp * dp * 16.0 >= 4294967296.0)     // (32-bit byte offsets from one base: m4q_session_create)
    return fail(M4Q_E_BADARG, "per-instance plant operators must stay below 4 GiB in total");
  const m4q::ShapeOps* sh = find_shape_any_order(p.dim_x, p.dim_u);
  if (!sh || sh->observe_kind != observe)
    return fail(M4Q_E_UNSUPPORTED, "m4q_session_set_observed_plant: no observed-plant kernel for dim_x=%d dim_u=%d", p.dim_x, p.dim_u);
  HIP_TRY(hipStreamSynchronize(s->stream));
  s->observe = 0;
  const Extent e0(B, plant_per_instance, dp * dp), ek(B, plant_per_instance, m * dp * dp);
  int rc;
  if ((rc = s->obs_op0.alloc(e0.count * C)) || (rc = s->obs_ops.alloc(ek.count * C)) || (rc = s->zs.alloc(B * (ns + 1) * np * C))) return rc;
  HIP_TRY(hipMemcpy(s->obs_op0.p, op0, e0.count * C, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(s->obs_ops.p, ops, ek.count * C, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(s->zs.p, 0, s->zs.bytes));
  HIP_TRY(hipMemcpy2D(s->zs.p, (ns + 1) * np * C, z0, np * C, np * C, B, hipMemcpyHostToDevice));
  // xs[:, 0] = observe(z0), by the kernel the loop calls
  m4q::ObserveArgs a{};
  a.B = s->B; a.kind = observe;
  a.z = (const cplx*)s->zs.p; a.z_stride = (long)((ns + 1) * np);
  a.x = (cplx*)s->f[M4Q_F_XS].p; a.x_stride = (long)((ns + 1) * n);
  rc = sh->launch_observe(a, s->stream);
  if (rc) return fail(rc, "observe kernel launch failed: %s", hipGetErrorString((hipError_t)(-rc)));
  HIP_TRY(hipStreamSynchronize(s->stream));
  s->obs_per = plant_per_instance != 0;
  s->obs_shape = sh;
  s->observe = observe;
  return 0;
}

int m4q_session_run_observed(m4q_session* s, int32_t step_begin, int32_t step_end) {
  if (!s || step_begin < 0 || step_end > s->prob.n_steps || step_begin >= step_end)
    return fail(M4Q_E_BADARG, "m4q_session_run_observed: bad step range [%d, %d)", step_begin, step_end);
  if (!s->observe) return fail(M4Q_E_BADARG, "m4q_session_run_observed: no observed plant is set (m4q_session_set_observed_plant)");
  const m4q_problem& p = s->prob;
  const size_t m = p.dim_u, dp = m4q::observe_dp(s->observe);
  m4q::ObsPlantArgs a{};
  a.B = s->B; a.kind = s->observe; a.n_steps = p.n_steps; a.dt = p.dt;
  a.codes = (const int*)s->f[M4Q_F_CODES].p; a.steps_done = (const int*)s->f[M4Q_F_STEPS_DONE].p;
  a.us = (const double*)s->f[M4Q_F_US].p;
  a.plant = plant_ops(s->obs_op0.p, s->obs_ops.p, s->B, s->obs_per, m, dp);
  a.zs = (cplx*)s->zs.p; a.xs = (cplx*)s->f[M4Q_F_XS].p;
  for (int k = step_begin; k < step_end; ++k) {
    if (int rc = m4q_session_run(s, k, k + 1)) return rc;
    a.step = k;
    const int rc = s->obs_shape->launch_observed_plant(a, s->stream);
    if (rc) return fail(rc, "observed-plant kernel launch failed: %s", hipGetErrorString((hipError_t)(-rc)));
  }
  return 0;
}

static int plant_states_copy(m4q_session* s, const char* who, void* host, size_t bytes, bool down) {
  if (!s || !host) return fail(M4Q_E_BADARG, "%s: bad argument", who);
  if (!s->observe) return fail(M4Q_E_BADARG, "%s: no observed plant is set (m4q_session_set_observed_plant)", who);
  if (bytes != s->zs.bytes) return fail(M4Q_E_BADARG, "%s: the plant states hold %zu bytes, got %zu", who, s->zs.bytes, bytes);
  if (down) HIP_TRY(hipMemcpyAsync(host, s->zs.p, bytes, hipMemcpyDeviceToHost, s->stream));
  else HIP_TRY(hipMemcpyAsync(s->zs.p, host, bytes, hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return check_watchdog(s);
}

int m4q_session_plant_states(m4q_session* s, void* host, size_t bytes) {
  return plant_states_copy(s, "m4q_session_plant_states", host, bytes, true);
}

int m4q_session_put_plant_states(m4q_session* s, const void* host, size_t bytes) {
  return plant_states_copy(s, "m4q_session_put_plant_states", const_cast<void*>(host), bytes, false);
}

int m4q_session_set_exit(m4q_session* s, int32_t mode, const double* W, const double* target, int32_t target_per_instance,
                         const double* thr, int32_t thr_per_instance) {
  if (!s) return fail(M4Q_E_BADARG, "m4q_session_set_exit: null session");
  const int side = mode & (M4Q_EXIT_PREV | M4Q_EXIT_NEXT), sense = mode & (M4Q_EXIT_BELOW | M4Q_EXIT_ABOVE);
  if (mode != 0 && ((mode & ~(M4Q_EXIT_PREV | M4Q_EXIT_NEXT | M4Q_EXIT_BELOW | M4Q_EXIT_ABOVE)) ||
                    (side != M4Q_EXIT_PREV && side != M4Q_EXIT_NEXT) || (sense != M4Q_EXIT_BELOW && sense != M4Q_EXIT_ABOVE)))
    return fail(M4Q_E_BADARG, "m4q_session_set_exit: mode 0x%x is not 0 or one of M4Q_EXIT_PREV / NEXT with one of M4Q_EXIT_BELOW / "
                "ABOVE", mode);
  if (mode != 0 && (!W || !target || !thr)) return fail(M4Q_E_BADARG, "m4q_session_set_exit: W, target and thr are required");
  if (mode != 0 && s->prob.plant_kind == M4Q_PLANT_NONE)
    return fail(M4Q_E_UNSUPPORTED, "m4q_session_set_exit: M4Q_PLANT_NONE sessions take their states from the host, which evaluates "
                "the exit condition itself");
  // a launch still in flight may read the buffers about to be replaced
  HIP_TRY(hipStreamSynchronize(s->stream));
  s->exit_mode = 0;
  s->exit_W.release(); s->exit_target.release(); s->exit_thr.release();
  if (mode == 0) return 0;
  const size_t n = s->prob.dim_x, B = s->B, C = 16;
  const size_t tb = Extent(B, target_per_instance, n).count * C, hb = Extent(B, thr_per_instance, 1).count * 8;
  int rc;
  if ((rc = s->exit_W.alloc(n * n * C)) || (rc = s->exit_target.alloc(tb)) || (rc = s->exit_thr.alloc(hb))) return rc;
  HIP_TRY(hipMemcpy(s->exit_W.p, W, n * n * C, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(s->exit_target.p, target, tb, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(s->exit_thr.p, thr, hb, hipMemcpyHostToDevice));
  s->exit_target_per = target_per_instance != 0;
  s->exit_thr_per = thr_per_instance != 0;
  s->exit_mode = mode;
  return 0;
}

static int check_noise_args(const char* who, int32_t mode, const double* sigma, size_t count) {
  if (mode != 0 && mode != M4Q_NOISE_IID && mode != M4Q_NOISE_HERMITIAN)
    return fail(M4Q_E_BADARG, "%s: mode %d is not 0, M4Q_NOISE_IID or M4Q_NOISE_HERMITIAN", who, mode);
  if (mode == 0) return 0;
  if (!sigma) return fail(M4Q_E_BADARG, "%s: sigma is required", who);
  for (size_t i = 0; i < count; ++i)
    if (!std::isfinite(sigma[i]) || sigma[i] < 0.0) return fail(M4Q_E_BADARG, "%s: sigma[%zu] = %g is not finite and >= 0", who, i, sigma[i]);
  return 0;
}

int m4q_session_set_noise(m4q_session* s, int32_t mode, const double* sigma, int32_t sigma_per_instance, uint64_t seed,
                          uint64_t member_base) {
  if (!s) return fail(M4Q_E_BADARG, "m4q_session_set_noise: null session");
  const size_t count = Extent(s->B, sigma_per_instance, 1).count;
  if (int rc = check_noise_args("m4q_session_set_noise", mode, sigma, count)) return rc;
  if (mode != 0 && s->prob.plant_kind == M4Q_PLANT_NONE)
    return fail(M4Q_E_BADARG, "m4q_session_set_noise: M4Q_PLANT_NONE sessions take their states from the host, which adds its own noise");
  if (mode == M4Q_NOISE_HERMITIAN && s->prob.plant_kind == M4Q_PLANT_PROCESS)
    return fail(M4Q_E_BADARG, "m4q_session_set_noise: M4Q_NOISE_HERMITIAN needs a density-matrix state; the loop state of "
                "M4Q_PLANT_PROCESS is a process vector (use M4Q_NOISE_IID)");
  if (s->ran && mode != s->noise_mode)
    return fail(M4Q_E_BADARG, "m4q_session_set_noise: the mode (%d) cannot change to %d after the session's first run: the arithmetic "
                "path depends on it (sigma, seed and member_base may)", s->noise_mode, mode);
  // a launch still in flight may read the buffer about to be replaced
  HIP_TRY(hipStreamSynchronize(s->stream));
  s->noise_mode = 0;
  s->noise_sigma.release();
  if (mode == 0) return 0;
  if (int rc = s->noise_sigma.alloc(count * 8)) return rc;
  HIP_TRY(hipMemcpy(s->noise_sigma.p, sigma, count * 8, hipMemcpyHostToDevice));
  s->noise_sigma_per = sigma_per_instance != 0;
  s->noise_seed = seed;
  s->noise_member_base = member_base;
  s->noise_mode = mode;
  return 0;
}

int m4q_session_sync(m4q_session* s) {
  if (!s) return fail(M4Q_E_BADARG, "m4q_session_sync: null session");
  HIP_TRY(hipStreamSynchronize(s->stream));
  return check_watchdog(s);
}

int m4q_session_set_codes(m4q_session* s, const int32_t* codes) {
  if (!s || !codes) return fail(M4Q_E_BADARG, "m4q_session_set_codes: bad argument");
  HIP_TRY(hipMemcpyAsync(s->f[M4Q_F_CODES].p, codes, (size_t)s->B * 4, hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return check_watchdog(s);
}

int m4q_session_kernel_ms(m4q_session* s, double* total_ms, int32_t* launches) {
  if (!s) return fail(M4Q_E_BADARG, "m4q_session_kernel_ms: null session");
  HIP_TRY(hipStreamSynchronize(s->stream));
  double tot = s->folded_ms;
  int n = s->folded_n;
  s->folded_ms = 0.0;
  s->folded_n = 0;
  for (auto& pr : s->pending) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, pr.first, pr.second));
    tot += ms;
    ++n;
    (void)hipEventDestroy(pr.first);
    (void)hipEventDestroy(pr.second);
  }
  s->pending.clear();
  if (total_ms) *total_ms = tot;
  if (launches) *launches = n;
  return check_watchdog(s);     // (timings of a launch that left through its watchdog are not handed out as if it had finished)
}

int m4q_session_qp_stats(m4q_session* s, int64_t* out6) {
  if (!s || !out6) return fail(M4Q_E_BADARG, "m4q_session_qp_stats: bad argument");
  HIP_TRY(hipStreamSynchronize(s->stream));
  unsigned long long q[24];
  HIP_TRY(hipMemcpy(q, s->queue.p, sizeof(q), hipMemcpyDeviceToHost));
  for (int i = 0; i < 6; ++i) out6[i] = (int64_t)q[1 + i];
  if (std::getenv("M4Q_QP_TRACE"))
    fprintf(stderr, "m4q: exact QP: %llu row sweeps in %llu wavefront passes (x4 rows = %llu): lane efficiency %.2f\n", q[2], q[7],
            4 * q[7], q[7] ? (double)q[2] / (4.0 * (double)q[7]) : 0.0);
  if (std::getenv("M4Q_PHASE_TRACE")) {          // -DM4Q_DEV_PHASE_CLOCK builds: wavefront time per phase of the main loop, 100 MHz ticks
    static const char* names[16] = {"draw/resume", "backward | exact: adjoint pass", "forward", "handover", "line search", "step done (plant)", "publish",
                                    "passes", "guess update", "passes with a line search",
                                    // (a name "a | b": a in a clipped kernel, b in an exact one.  Slots 10, 11 and 13 are parts of "step done"
                                    //  in a clipped kernel - slot 5 is then the rest of it, the passes in which no row ends a step)
                                    "step: bookkeeping, us | exact: pinned sweep", "step: plant to xs | exact: policy rollout",
                                    "exact: ratio rollout", "step: exit, rest | exact: blend", "exact: open rollout",
                                    "exact: bookkeeping + copies"};
    unsigned long long tot = 0;
    for (int i = 0; i < 16; ++i) tot += (i == 7 || i == 9) ? 0 : q[8 + i];
    for (int i = 0; i < 16; ++i)
      fprintf(stderr, "m4q phase %-44s %14llu %s  %5.1f %%\n", names[i], q[8 + i], (i == 7 || i == 9) ? "     " : "ticks",
              (i != 7 && i != 9 && tot) ? 100.0 * (double)q[8 + i] / (double)tot : 0.0);
  }
  return check_watchdog(s);
}

int m4q_session_info(const m4q_session* s, int64_t* hbm_bytes, int32_t* grid, int32_t* lds_bytes) {
  if (!s) return fail(M4Q_E_BADARG, "m4q_session_info: null session");
  int64_t tot = 0;
  for (int i = 0; i < M4Q_F_COUNT; ++i) tot += (int64_t)s->f[i].bytes;
  tot += (int64_t)(s->wsXg.bytes + s->wsUg.bytes + s->wsG.bytes);
  if (hbm_bytes) *hbm_bytes = tot;
  const m4q::Path path = s->path();
  if (grid) *grid = path == m4q::PATH_SG ? s->grid_sg : s->grid;
  if (lds_bytes) *lds_bytes = s->mpc_ops->mpc_lds_bytes(s->prob.plant_kind, path, (s->prob.qp_flags & M4Q_QP_EXACT_BOX) != 0);
  return 0;
}

// ------------------------------------------------------------------------------------------
// one-shot host entry points
// ------------------------------------------------------------------------------------------
int m4q_linearize_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t order, int32_t T, const double* models,
                        int32_t model_per_instance, const double* X, const double* U, double* A_ls, double* B_ls,
                        double* Delta_ls) {
  const m4q::ShapeOps* sh = find_shape(dim_x, dim_u, order);
  if (!sh) return fail(M4Q_E_UNSUPPORTED, "no kernel for dim_x=%d dim_u=%d order=%d", dim_x, dim_u, order);
  if (B <= 0 || T <= 0 || !models || !X || !U || !A_ls || !B_ls || !Delta_ls) return fail(M4Q_E_BADARG, "m4q_linearize_batch: bad argument");
  if (int rc = need_device()) return rc;
  const size_t n = dim_x, m = dim_u, P = sh->np, BT = (size_t)B * T;
  const Extent mdl(B, model_per_instance, n * n * (1 + P));
  Stage st;
  m4q::LinArgs a{};
  a.B = B; a.T = T;
  a.models = st.in<cplx>(models, mdl.count); a.model_stride = mdl.stride;
  a.X = st.in<cplx>(X, BT * n); a.U = st.in<double>(U, BT * m);
  a.A_ls = st.out<cplx>(A_ls, BT * n * n); a.B_ls = st.out<cplx>(B_ls, BT * n * m); a.D_ls = st.out<cplx>(Delta_ls, BT * n);
  if (st.error()) return st.error();
  return st.finish(sh->launch_linearize(a, nullptr), "linearize");
}

int m4q_quad_program_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t T, int32_t qp_flags, double sat, double du,
                           const double* x_init, const double* X_bm, const double* U_bm, int32_t bm_per_instance,
                           const double* Q_ls, const double* R_ls, const double* A_ls, const double* B_ls,
                           const double* Delta_ls, const double* u_prev, double* X_opt, double* U_opt, double* cost,
                           double* gains) {
  const m4q::ShapeOps* sh = find_shape_any_order(dim_x, dim_u);
  if (!sh) return fail(M4Q_E_UNSUPPORTED, "no kernel for dim_x=%d dim_u=%d", dim_x, dim_u);
  if (B <= 0 || T <= 0 || !x_init || !X_bm || !U_bm || !Q_ls || !R_ls || !A_ls || !B_ls || !X_opt || !U_opt || !cost)
    return fail(M4Q_E_BADARG, "m4q_quad_program_batch: bad argument");
  if (!(sat > 0)) return fail(M4Q_E_BADARG, "sat must be positive");
  if (int rc = check_qp_flags(qp_flags)) return rc;
  if (int rc = need_device()) return rc;
  const size_t n = dim_x, m = dim_u, BT = (size_t)B * T, BT1 = (size_t)B * (T + 1);
  const Extent xbm(B, bm_per_instance, (size_t)(T + 1) * n), ubm(B, bm_per_instance, (size_t)T * m);
  Stage st;
  m4q::QpArgs a{};
  a.B = B; a.T = T; a.flags = qp_flags; a.sat = sat; a.du = du;
  a.x_init = st.in<cplx>(x_init, (size_t)B * n);
  a.X_bm = st.in<cplx>(X_bm, xbm.count); a.xbm_stride = xbm.stride;
  a.U_bm = st.in<double>(U_bm, ubm.count); a.ubm_stride = ubm.stride;
  a.Q_ls = st.in<cplx>(Q_ls, (size_t)(T + 1) * n * n); a.R_ls = st.in<cplx>(R_ls, (size_t)T * m * m);
  a.A_ls = st.in<cplx>(A_ls, BT * n * n); a.B_ls = st.in<cplx>(B_ls, BT * n * m);
  if (Delta_ls) a.D_ls = st.in<cplx>(Delta_ls, BT * n);
  if (u_prev) a.u_prev = st.in<double>(u_prev, (size_t)B * m);
  std::vector<int> sweeps;                                  // diagnostic (M4Q_QP_TRACE): pinned sweeps per instance
  if (qp_flags & M4Q_QP_EXACT_BOX) {
    if (st.error()) return st.error();
    if ((double)BT1 * n * 16 * 2 >= 4294967296.0)
      return fail(M4Q_E_BADARG, "M4Q_QP_EXACT_BOX: batch too large for one call (trajectory workspace must stay below 4 GiB)");
    if (getenv("M4Q_QP_TRACE")) {
      sweeps.resize(B);
      a.sweep_counts = st.out<int>(sweeps.data(), B);
    }
    a.X_alt = st.out<cplx>(nullptr, 2 * BT1 * n); a.U_alt = st.out<double>(nullptr, 2 * BT * m);
    a.pin_stat = st.out<double>(nullptr, BT * m);
  }
  a.X_opt = st.out<cplx>(X_opt, BT1 * n); a.U_opt = st.out<double>(U_opt, BT * m); a.cost = st.out<double>(cost, B);
  a.gains = st.out<cplx>(gains, BT * (n + 1) * m);          // (workspace when the caller wants no gains)
  if (st.error()) return st.error();
  const int rc = st.finish(sh->launch_qp(a, nullptr), "qp");
  if (!rc && !sweeps.empty()) {
    long sum = 0;
    int mx = 0;
    for (int v : sweeps) { sum += v; mx = v > mx ? v : mx; }
    fprintf(stderr, "m4q: exact box QP: %d instances, pinned sweeps mean %.2f max %d\n", B, (double)sum / B, mx);
  }
  return rc;
}

int m4q_noise_sample_batch(int32_t B, int32_t n, int32_t mode, const double* sigma, int32_t sigma_per_instance, uint64_t seed,
                           uint64_t member_base, int32_t state_index, double* out) {
  if (B <= 0 || n <= 0 || !out || mode == 0 || state_index < 1)
    return fail(M4Q_E_BADARG, "m4q_noise_sample_batch: bad argument (B, n >= 1, a noise mode, state_index >= 1, out)");
  const Extent sg(B, sigma_per_instance, 1);
  if (int rc = check_noise_args("m4q_noise_sample_batch", mode, sigma, sg.count)) return rc;
  const m4q::ShapeOps* sh = nullptr;
  for (int nu = 1; nu <= 3 && !sh; ++nu) sh = find_shape_any_order(n, nu, true);
  if (!sh) return fail(M4Q_E_UNSUPPORTED, "m4q_noise_sample_batch: no compiled kernel with dim_x=%d", n);
  if (mode == M4Q_NOISE_HERMITIAN && sh->d * sh->d != n)
    return fail(M4Q_E_BADARG, "m4q_noise_sample_batch: M4Q_NOISE_HERMITIAN needs n = d d, got n = %d", n);
  if (int rc = need_device()) return rc;
  Stage st;
  m4q::NoiseArgs a{};
  a.B = B; a.mode = mode; a.state_index = (unsigned)state_index; a.seed = seed; a.member_base = member_base;
  a.sigma = st.in<double>(sigma, sg.count); a.sigma_stride = sg.stride;
  a.out = st.out<cplx>(out, (size_t)B * n);
  if (st.error()) return st.error();
  const int rc = sh->launch_noise(a, nullptr);
  if (rc) return fail(rc, "noise kernel launch failed: %s", hipGetErrorString((hipError_t)(-rc)));    // (this one names the reason)
  return st.finish(0, "noise kernel");
}

int m4q_discretize_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t order, double dt, const double* generators,
                         int32_t gen_per_instance, const double* scales, double* models) {
  const m4q::ShapeOps* sh = find_shape(dim_x, dim_u, order);
  if (!sh) return fail(M4Q_E_UNSUPPORTED, "no kernel for dim_x=%d dim_u=%d order=%d", dim_x, dim_u, order);
  if (B <= 0 || !generators || !models) return fail(M4Q_E_BADARG, "m4q_discretize_batch: bad argument");
  if (order > 2)
    return fail(M4Q_E_UNSUPPORTED, "m4q_discretize_batch: the device discretisation covers orders 1 and 2 (order %d: use the host "
                "discretize_homogeneous and upload the models)", order);
  if (int rc = need_device()) return rc;
  const size_t n = dim_x, m = dim_u, P = sh->np;
  const Extent gen(B, gen_per_instance, (1 + m) * n * n);
  Stage st;
  m4q::DiscArgs a{};
  a.B = B; a.dt = dt;
  a.gens = st.in<cplx>(generators, gen.count); a.gen_stride = gen.stride;
  if (scales) a.scales = st.in<double>(scales, (size_t)B * (1 + m));
  a.models = st.out<cplx>(models, (size_t)B * n * n * (1 + P));
  if (st.error()) return st.error();
  return st.finish(sh->launch_discretize(a, m4q::COORDS_COMPLEX, nullptr), "discretize");
}

int m4q_session_build_models(m4q_session* s, double dt, const double* generators, int32_t gen_per_instance,
                             const double* scales) {
  if (!s || !generators) return fail(M4Q_E_BADARG, "m4q_session_build_models: bad argument");
  const m4q_problem& p = s->prob;
  if (p.order > 2)
    return fail(M4Q_E_UNSUPPORTED, "m4q_session_build_models: the device discretisation covers orders 1 and 2 (order %d: build the "
                "models with the host discretize_homogeneous and upload them)", p.order);
  const size_t n = p.dim_x, m = p.dim_u, P = s->shape->np;
  const size_t nset = gen_per_instance ? (size_t)s->B : 1;
  const size_t nmodels = p.model_per_instance ? (size_t)s->B : 1;
  if ((gen_per_instance || scales) && !p.model_per_instance)
    return fail(M4Q_E_BADARG, "per-instance generators or scales need model_per_instance = 1");
  const Extent gen(s->B, gen_per_instance, (1 + m) * n * n);
  Stage st;                                  // (inputs only: the launches go to the session's stream, the models stay on the device)
  m4q::DiscArgs a{};
  a.B = (int)nmodels; a.dt = dt;
  a.gens = st.in<cplx>(generators, gen.count); a.gen_stride = gen.stride;
  if (scales) a.scales = st.in<double>(scales, (size_t)s->B * (1 + m));
  if (st.error()) return st.error();
  a.models = s->f[M4Q_F_MODELS].p;
  int rc = s->shape->launch_discretize(a, m4q::COORDS_COMPLEX, s->stream);
  if (rc) return fail(rc, "discretize launch failed");
  s->sg_ok = false;
  s->copies[m4q::COORDS_HERM][M4Q_F_MODELS].ok = s->copies[m4q::COORDS_TRACELESS][M4Q_F_MODELS].ok = false;
  if (s->allowed[m4q::PATH_REAL]) {
    // the same expansion on the real coordinate systems: lift the generators (few, or one set per member).  Generators that leave
    // the trace coordinate alone (row 0 and column 0 of O^T G O zero: trace-preserving and unital, every -i[H, .] is) have
    // block-diagonal products, so the expansion of their (n-1) x (n-1) blocks IS the traceless block of the model
    const Lift L = lift_blocks(s->shape->d, reinterpret_cast<const std::complex<double>*>(generators), nset * (1 + m), 1, false,
                               s->allowed[m4q::PATH_TRACELESS]);
    for (m4q::Coords c : {m4q::COORDS_HERM, m4q::COORDS_TRACELESS}) {
      if (!L.ok[c]) continue;
      const size_t k = c == m4q::COORDS_HERM ? n : n - 1;
      m4q_session::Copy& dst = s->copies[c][M4Q_F_MODELS];
      m4q::DiscArgs r = a;
      r.gens = st.in<double>(L.v[c].data(), L.v[c].size());
      r.gen_stride = Extent(s->B, gen_per_instance, (1 + m) * k * k).stride;
      if (st.error()) return st.error();
      if ((rc = dst.buf.alloc(nmodels * k * k * (1 + P) * 8))) return rc;
      r.models = dst.buf.p;
      rc = s->shape->launch_discretize(r, c, s->stream);
      if (rc) return fail(rc, "discretize launch failed");
      dst.ok = true;
    }
    // shared-generator form (PATH_SG): ONE generator set, order 1 - member i's model is [I + dt s_i0 L_0 | dt s_ik L_k]; keep dt L_k
    // on the traceless coordinates and the scales (ones when none were given)
    if (L.ok[m4q::COORDS_TRACELESS] && s->allowed[m4q::PATH_SG] && !gen_per_instance && p.model_per_instance) {
      const std::vector<double>& blocks = L.v[m4q::COORDS_TRACELESS];
      std::vector<double> g(blocks.size());
      for (size_t e = 0; e < blocks.size(); ++e) g[e] = dt * blocks[e];
      std::vector<double> sc((size_t)s->B * (1 + m), 1.0);
      if (scales) std::copy(scales, scales + sc.size(), sc.begin());
      if ((rc = s->sg_gens.alloc(g.size() * 8)) || (rc = s->sg_scales.alloc(sc.size() * 8))) return rc;
      HIP_TRY(hipMemcpy(s->sg_gens.p, g.data(), g.size() * 8, hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(s->sg_scales.p, sc.data(), sc.size() * 8, hipMemcpyHostToDevice));
      s->sg_ok = true;
    }
  }
  HIP_TRY(hipStreamSynchronize(s->stream));
  return 0;
}

int m4q_plant_step_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t plant_kind, double dt, const double* x,
                         const double* u, const double* op0, const double* ops, int32_t plant_per_instance,
                         double* x_next) {
  const m4q::ShapeOps* sh = find_shape_any_order(dim_x, dim_u, /*plant_ok=*/true);
  if (!sh) return fail(M4Q_E_UNSUPPORTED, "no kernel for dim_x=%d dim_u=%d", dim_x, dim_u);
  if (B <= 0 || !x || !u || !op0 || !ops || !x_next) return fail(M4Q_E_BADARG, "m4q_plant_step_batch: bad argument");
  if (int rc = check_device_plant_kind(plant_kind, dim_x, "m4q_plant_step_batch: bad argument")) return rc;
  if (int rc = need_device()) return rc;
  const size_t n = dim_x, m = dim_u;
  Stage st;
  m4q::PlantArgs a{};
  a.B = B; a.kind = plant_kind; a.dt = dt;
  a.x = st.in<cplx>(x, (size_t)B * n); a.u = st.in<double>(u, (size_t)B * m);
  a.plant = stage_plant(st, B, plant_kind, dim_x, dim_u, op0, ops, plant_per_instance);
  a.x_next = st.out<cplx>(x_next, (size_t)B * n);
  if (st.error()) return st.error();
  return st.finish(sh->launch_plant(a, nullptr), "plant");
}

namespace {
// the arguments the two rollouts share, checked before a device is asked for
int check_roll_args(const char* who, int32_t B, int32_t N, const double* x0, const double* u, const double* W, const double* target,
                    int32_t xs_mode, double* xs, int32_t q_mode, double* q) {
  if (B < 1 || N < 1) return fail(M4Q_E_BADARG, "%s: B and N must be at least 1 (got %d, %d)", who, B, N);
  if (!x0 || !u) return fail(M4Q_E_BADARG, "%s: x0 and u are required", who);
  if (xs_mode < 0 || xs_mode > 2 || q_mode < 0 || q_mode > 2)
    return fail(M4Q_E_BADARG, "%s: xs_mode and q_mode are 0 (none), 1 (last) or 2 (all), got %d and %d", who, xs_mode, q_mode);
  if (xs_mode == 0 && q_mode == 0) return fail(M4Q_E_BADARG, "%s: nothing to return (xs_mode and q_mode are both 0)", who);
  if (xs_mode != 0 && !xs) return fail(M4Q_E_BADARG, "%s: xs_mode %d without xs", who, xs_mode);
  if (q_mode != 0 && (!q || !W || !target)) return fail(M4Q_E_BADARG, "%s: q_mode %d needs W, target and q", who, q_mode);
  return 0;
}

// stages what the two rollouts share
m4q::RollArgs stage_roll(Stage& st, int32_t B, size_t n, size_t m, int32_t N, const double* x0, const double* u, int32_t u_per_instance,
                         const double* u_scale, const double* W, const double* target, int32_t target_per_instance, int32_t xs_mode,
                         double* xs, int32_t q_mode, double* q) {
  const Extent eu(B, u_per_instance, (size_t)N * m), ef(B, target_per_instance, n);
  m4q::RollArgs a{};
  a.B = B; a.N = N; a.xs_mode = xs_mode; a.q_mode = q_mode;
  a.x0 = st.in<cplx>(x0, (size_t)B * n);
  a.u = st.in<double>(u, eu.count); a.u_stride = eu.stride;
  if (u_scale) a.u_scale = st.in<double>(u_scale, (size_t)B * m);
  if (q_mode != 0) {
    a.W = st.in<cplx>(W, n * n);
    a.target = st.in<cplx>(target, ef.count); a.target_stride = ef.stride;
  }
  if (xs_mode != 0) a.xs = st.out<cplx>(xs, (size_t)B * (xs_mode == 2 ? (size_t)N + 1 : 1) * n);
  if (q_mode != 0) a.q = st.out<double>(q, (size_t)B * (q_mode == 2 ? (size_t)N + 1 : 1));
  return a;
}
}  // namespace

int m4q_plant_rollout_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t plant_kind, int32_t N, const double* dts,
                            const double* x0, const double* u, int32_t u_per_instance, const double* u_scale, const double* op0,
                            const double* ops, int32_t plant_per_instance, const double* W, const double* target,
                            int32_t target_per_instance, int32_t xs_mode, double* xs, int32_t q_mode, double* q) {
  const char* who = "m4q_plant_rollout_batch";
  const m4q::ShapeOps* sh = nullptr;
  if (int rc = plant_shape(who, /*named=*/false, dim_x, dim_u, /*needs_qp=*/false, &sh)) return rc;
  if (int rc = check_roll_args(who, B, N, x0, u, W, target, xs_mode, xs, q_mode, q)) return rc;
  if (!dts || !op0 || !ops) return fail(M4Q_E_BADARG, "%s: dts, op0 and ops are required", who);
  if (int rc = check_plant_kind(who, /*named=*/false, plant_kind, dim_x, nullptr, nullptr)) return rc;
  if (int rc = need_device()) return rc;
  Stage st;
  m4q::RollArgs a = stage_roll(st, B, dim_x, dim_u, N, x0, u, u_per_instance, u_scale, W, target, target_per_instance, xs_mode, xs, q_mode, q);
  a.kind = plant_kind;
  a.dts = st.in<double>(dts, N);
  a.plant = stage_plant(st, B, plant_kind, dim_x, dim_u, op0, ops, plant_per_instance);
  if (st.error()) return st.error();
  return st.finish(sh->launch_plant_rollout(a, nullptr), "plant rollout");
}

int m4q_model_rollout_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t order, int32_t N, const double* x0, const double* u,
                            int32_t u_per_instance, const double* u_scale, const double* models, int32_t model_per_instance,
                            const double* W, const double* target, int32_t target_per_instance, int32_t xs_mode, double* xs,
                            int32_t q_mode, double* q) {
  const m4q::ShapeOps* sh = find_shape(dim_x, dim_u, order);
  if (!sh) return fail(M4Q_E_UNSUPPORTED, "no model kernel for dim_x=%d dim_u=%d order=%d", dim_x, dim_u, order);
  if (int rc = check_roll_args("m4q_model_rollout_batch", B, N, x0, u, W, target, xs_mode, xs, q_mode, q)) return rc;
  if (!models) return fail(M4Q_E_BADARG, "m4q_model_rollout_batch: models are required");
  if (int rc = need_device()) return rc;
  const size_t n = dim_x, m = dim_u, P = sh->np;
  const Extent mdl(B, model_per_instance, n * n * (1 + P));
  Stage st;
  m4q::RollArgs a = stage_roll(st, B, n, m, N, x0, u, u_per_instance, u_scale, W, target, target_per_instance, xs_mode, xs, q_mode, q);
  a.models = st.in<cplx>(models, mdl.count); a.model_stride = mdl.stride;
  if (st.error()) return st.error();
  return st.finish(sh->launch_model_rollout(a, nullptr), "model rollout");
}

namespace {
// the arguments the two feedback runs share, checked before a device is asked for
int check_feedback_args(const char* who, int32_t B, int32_t dim_x, int32_t N, const double* x0, const double* gains, const double* x_ref,
                        const double* u_ref, double sat, int32_t du_band, double du, const double* u_prev, int32_t noise_mode,
                        const double* sigma, size_t sigma_count, bool hermitian_ok, const double* W, const double* target, int32_t xs_mode,
                        double* xs, int32_t q_mode, double* q, double* us, int32_t* clipped, int32_t* status) {
  if (B < 1 || N < 1) return fail(M4Q_E_BADARG, "%s: B and N must be at least 1 (got %d, %d)", who, B, N);
  if (!x0 || !gains || !x_ref || !u_ref || !status) return fail(M4Q_E_BADARG, "%s: x0, gains, x_ref, u_ref and status are required", who);
  if (!(sat > 0.0)) return fail(M4Q_E_BADARG, "%s: sat = %g is not positive (INFINITY: no box)", who, sat);
  if (du_band && !(du > 0.0 && std::isfinite(du))) return fail(M4Q_E_BADARG, "%s: du = %g is not positive and finite", who, du);
  if (du_band && !u_prev) return fail(M4Q_E_BADARG, "%s: the band needs u_prev, the control applied before step 0", who);
  if (xs_mode < 0 || xs_mode > 2 || q_mode < 0 || q_mode > 2)
    return fail(M4Q_E_BADARG, "%s: xs_mode and q_mode are 0 (none), 1 (last) or 2 (all), got %d and %d", who, xs_mode, q_mode);
  if (xs_mode == 0 && q_mode == 0 && !us && !clipped)
    return fail(M4Q_E_BADARG, "%s: nothing to return (xs_mode and q_mode are 0, us and clipped NULL)", who);
  if (xs_mode != 0 && !xs) return fail(M4Q_E_BADARG, "%s: xs_mode %d without xs", who, xs_mode);
  if (q_mode != 0 && (!q || !W || !target)) return fail(M4Q_E_BADARG, "%s: q_mode %d needs W, target and q", who, q_mode);
  if (int rc = check_noise_args(who, noise_mode, sigma, sigma_count)) return rc;
  if (noise_mode == M4Q_NOISE_HERMITIAN && !hermitian_ok)
    return fail(M4Q_E_BADARG, "%s: M4Q_NOISE_HERMITIAN needs a density-matrix state, n = d d and no process plant (dim_x = %d: use "
                "M4Q_NOISE_IID)", who, dim_x);
  return 0;
}

// stages what the two feedback runs share: the rollout with u_ref in its controls' place, the law, the noise, the further outputs
m4q::FeedbackArgs stage_feedback(Stage& st, int32_t B, size_t n, size_t m, int32_t N, const double* x0, const double* gains,
                                 const double* x_ref, const double* u_ref, int32_t law_per_instance, double sat, int32_t du_band, double du,
                                 const double* u_prev, int32_t u_prev_per_instance, const double* u_scale, int32_t noise_mode,
                                 const double* sigma, int32_t sigma_per_instance, uint64_t seed, uint64_t member_base, const double* W,
                                 const double* target, int32_t target_per_instance, int32_t xs_mode, double* xs, int32_t q_mode, double* q,
                                 double* us, int32_t* clipped, int32_t* status) {
  m4q::FeedbackArgs f{};
  f.roll = stage_roll(st, B, n, m, N, x0, u_ref, law_per_instance, u_scale, W, target, target_per_instance, xs_mode, xs, q_mode, q);
  const Extent eg(B, law_per_instance, (size_t)N * (n + 1) * m), ex(B, law_per_instance, (size_t)N * n);
  f.u_ref = f.roll.u;
  f.gains = st.in<cplx>(gains, eg.count);
  f.x_ref = st.in<cplx>(x_ref, ex.count);
  f.law_per = law_per_instance ? 1 : 0;
  f.sat = sat; f.du_band = du_band ? 1 : 0; f.du = du_band ? du : 0.0;
  if (du_band) {
    const Extent ep(B, u_prev_per_instance, m);
    f.u_prev = st.in<double>(u_prev, ep.count); f.u_prev_stride = ep.stride;
  }
  f.noise_mode = noise_mode; f.seed = seed; f.member_base = member_base;
  if (noise_mode != 0) {
    const Extent sg(B, sigma_per_instance, 1);
    f.sigma = st.in<double>(sigma, sg.count); f.sigma_stride = sg.stride;
  }
  if (us) f.us = st.out<double>(us, (size_t)B * N * m);
  if (clipped) f.clipped = st.out<int>(clipped, (size_t)B);
  f.status = st.out<int>(status, (size_t)B);
  return f;
}
}  // namespace

int m4q_plant_feedback_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t plant_kind, int32_t N, const double* dts, const double* x0,
                             const double* gains, const double* x_ref, const double* u_ref, int32_t law_per_instance, double sat,
                             int32_t du_band, double du, const double* u_prev, int32_t u_prev_per_instance, const double* u_scale,
                             const double* op0, const double* ops, int32_t plant_per_instance, int32_t noise_mode, const double* sigma,
                             int32_t sigma_per_instance, uint64_t seed, uint64_t member_base, const double* W, const double* target,
                             int32_t target_per_instance, int32_t xs_mode, double* xs, int32_t q_mode, double* q, double* us,
                             int32_t* clipped, int32_t* status) {
  const char* who = "m4q_plant_feedback_batch";
  const m4q::ShapeOps* sh = nullptr;
  if (int rc = plant_shape(who, /*named=*/false, dim_x, dim_u, /*needs_qp=*/false, &sh)) return rc;
  const size_t sigma_count = B < 1 ? 0 : Extent(B, sigma_per_instance, 1).count;
  if (int rc = check_feedback_args(who, B, dim_x, N, x0, gains, x_ref, u_ref, sat, du_band, du, u_prev, noise_mode, sigma, sigma_count,
                                   plant_kind != M4Q_PLANT_PROCESS, W, target, xs_mode, xs, q_mode, q, us, clipped, status))
    return rc;
  if (!dts || !op0 || !ops) return fail(M4Q_E_BADARG, "%s: dts, op0 and ops are required", who);
  if (int rc = check_plant_kind(who, /*named=*/false, plant_kind, dim_x, nullptr, nullptr)) return rc;
  if (int rc = need_device()) return rc;
  Stage st;
  m4q::FeedbackArgs a = stage_feedback(st, B, dim_x, dim_u, N, x0, gains, x_ref, u_ref, law_per_instance, sat, du_band, du, u_prev,
                                       u_prev_per_instance, u_scale, noise_mode, sigma, sigma_per_instance, seed, member_base, W, target,
                                       target_per_instance, xs_mode, xs, q_mode, q, us, clipped, status);
  a.roll.kind = plant_kind;
  a.roll.dts = st.in<double>(dts, N);
  a.roll.plant = stage_plant(st, B, plant_kind, dim_x, dim_u, op0, ops, plant_per_instance);
  if (st.error()) return st.error();
  return st.finish(sh->launch_plant_feedback(a, nullptr), "plant feedback");
}

int m4q_model_feedback_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t order, int32_t N, const double* x0, const double* gains,
                             const double* x_ref, const double* u_ref, int32_t law_per_instance, double sat, int32_t du_band, double du,
                             const double* u_prev, int32_t u_prev_per_instance, const double* u_scale, const double* models,
                             int32_t model_per_instance, int32_t noise_mode, const double* sigma, int32_t sigma_per_instance, uint64_t seed,
                             uint64_t member_base, const double* W, const double* target, int32_t target_per_instance, int32_t xs_mode,
                             double* xs, int32_t q_mode, double* q, double* us, int32_t* clipped, int32_t* status) {
  const char* who = "m4q_model_feedback_batch";
  const m4q::ShapeOps* sh = find_shape(dim_x, dim_u, order);
  if (!sh) return fail(M4Q_E_UNSUPPORTED, "no model kernel for dim_x=%d dim_u=%d order=%d", dim_x, dim_u, order);
  const size_t sigma_count = B < 1 ? 0 : Extent(B, sigma_per_instance, 1).count;
  if (int rc = check_feedback_args(who, B, dim_x, N, x0, gains, x_ref, u_ref, sat, du_band, du, u_prev, noise_mode, sigma, sigma_count,
                                   dim_d(dim_x) != 0, W, target, xs_mode, xs, q_mode, q, us, clipped, status))
    return rc;
  if (!models) return fail(M4Q_E_BADARG, "%s: models are required", who);
  if (int rc = need_device()) return rc;
  const size_t n = dim_x, m = dim_u, P = sh->np;
  const Extent mdl(B, model_per_instance, n * n * (1 + P));
  Stage st;
  m4q::FeedbackArgs a = stage_feedback(st, B, n, m, N, x0, gains, x_ref, u_ref, law_per_instance, sat, du_band, du, u_prev,
                                       u_prev_per_instance, u_scale, noise_mode, sigma, sigma_per_instance, seed, member_base, W, target,
                                       target_per_instance, xs_mode, xs, q_mode, q, us, clipped, status);
  a.roll.models = st.in<cplx>(models, mdl.count); a.roll.model_stride = mdl.stride;
  if (st.error()) return st.error();
  return st.finish(sh->launch_model_feedback(a, nullptr), "model feedback");
}

namespace {
// the arguments the two rollout gradients share, checked before a device is asked for
int check_grad_args(const char* who, int32_t B, int32_t N, const double* x0, const double* u, int32_t u_per_instance, const double* W,
                    const double* target, int32_t q_mode, const double* weights, int32_t reduce, double* q, double* grad, double* q_mean) {
  if (B < 1 || N < 1) return fail(M4Q_E_BADARG, "%s: B and N must be at least 1 (got %d, %d)", who, B, N);
  if (!x0 || !u || !W || !target) return fail(M4Q_E_BADARG, "%s: x0, u, W and target are required", who);
  if (q_mode < 1 || q_mode > 2) return fail(M4Q_E_BADARG, "%s: q_mode is 1 (J = q_N) or 2 (J = sum_t q_t), got %d", who, q_mode);
  if (!q || !grad) return fail(M4Q_E_BADARG, "%s: q and grad are required", who);
  if (reduce && u_per_instance) return fail(M4Q_E_BADARG, "%s: reduce needs one control sequence shared by the ensemble (u_per_instance 0)", who);
  if (reduce && !q_mean) return fail(M4Q_E_BADARG, "%s: reduce needs q_mean", who);
  if (weights)
    for (int32_t b = 0; b < B; ++b)
      if (!std::isfinite(weights[b]) || weights[b] < 0.0) return fail(M4Q_E_BADARG, "%s: weights[%d] = %g is not a finite non-negative number", who, b, weights[b]);
  return 0;
}

// stages what the two rollout gradients share: the rollout with every state kept in a workspace, the outputs, the reduction's buffers
m4q::GradArgs stage_grad(Stage& st, int32_t B, size_t n, size_t m, int32_t N, const double* x0, const double* u, int32_t u_per_instance,
                         const double* u_scale, const double* W, const double* target, int32_t target_per_instance, int32_t q_mode,
                         const double* weights, int32_t reduce, double* q, double* grad, double* grad_scale, double* q_mean) {
  m4q::GradArgs g{};
  g.roll = stage_roll(st, B, n, m, N, x0, u, u_per_instance, u_scale, W, target, target_per_instance, /*xs_mode=*/2, /*xs=*/nullptr, q_mode, q);
  const size_t nm = (size_t)N * m;
  g.grad = st.out<double>(reduce ? nullptr : grad, (size_t)B * nm);       // (with reduce the members' gradients stay on the device)
  if (grad_scale) g.grad_scale = st.out<double>(grad_scale, (size_t)B * m);
  g.reduce = reduce ? 1 : 0;
  if (reduce) {
    std::vector<double> w;
    if (weights) w.assign(weights, weights + B);
    else w.assign((size_t)B, 1.0 / B);
    g.weights = st.in<double>(w.data(), (size_t)B);
    g.partial = st.out<double>(nullptr, (((size_t)B + m4q::GRAD_CHUNK - 1) / m4q::GRAD_CHUNK) * (nm + 1));
    g.grad_mean = st.out<double>(grad, nm);
    g.q_mean = st.out<double>(q_mean, 1);
  }
  return g;
}
}  // namespace

int m4q_plant_rollout_grad_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t plant_kind, int32_t N, const double* dts,
                                 const double* x0, const double* u, int32_t u_per_instance, const double* u_scale, const double* op0,
                                 const double* ops, int32_t plant_per_instance, const double* W, const double* target,
                                 int32_t target_per_instance, int32_t q_mode, const double* weights, int32_t reduce, double* q,
                                 double* grad, double* grad_scale, double* q_mean) {
  const char* who = "m4q_plant_rollout_grad_batch";
  const m4q::ShapeOps* sh = nullptr;
  if (int rc = plant_shape(who, /*named=*/false, dim_x, dim_u, /*needs_qp=*/false, &sh)) return rc;
  if (int rc = check_grad_args(who, B, N, x0, u, u_per_instance, W, target, q_mode, weights, reduce, q, grad, q_mean)) return rc;
  if (!dts || !op0 || !ops) return fail(M4Q_E_BADARG, "%s: dts, op0 and ops are required", who);
  if (int rc = check_plant_kind(who, /*named=*/false, plant_kind, dim_x, "gradient kernel",
                                "take the gradient of the discretised model with m4q_model_rollout_grad_batch"))
    return rc;
  if (int rc = need_device()) return rc;
  Stage st;
  m4q::GradArgs a = stage_grad(st, B, dim_x, dim_u, N, x0, u, u_per_instance, u_scale, W, target, target_per_instance, q_mode, weights, reduce,
                               q, grad, grad_scale, q_mean);
  a.roll.kind = plant_kind;
  a.roll.dts = st.in<double>(dts, N);
  a.roll.plant = stage_plant(st, B, plant_kind, dim_x, dim_u, op0, ops, plant_per_instance);
  if (st.error()) return st.error();
  return st.finish(sh->launch_plant_grad(a, nullptr), "plant rollout gradient");
}

int m4q_plant_rollout_param_grad_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t plant_kind, int32_t N, const double* dts,
                                       const double* x0, const double* u, int32_t u_per_instance, const double* u_scale,
                                       const double* op0, const double* ops, int32_t plant_per_instance, int32_t p, const double* dirs,
                                       int32_t dirs_per_instance, const double* W, const double* data, int32_t data_per_instance,
                                       const double* col_w, double* J, double* grad_theta, double* grad_scale) {
  const char* who = "m4q_plant_rollout_param_grad_batch";
  const m4q::ShapeOps* sh = nullptr;
  if (int rc = plant_shape(who, /*named=*/true, dim_x, dim_u, /*needs_qp=*/false, &sh)) return rc;
  if (sh->plant_only)
    return fail(M4Q_E_UNSUPPORTED, "%s: dim_x=%d dim_u=%d is a plant-only shape, it has no parameter-gradient kernel", who, dim_x, dim_u);
  sh = find_shape(dim_x, dim_u, 1);        // (the kernels do not depend on the library order: the order-1 object holds them)
  if (!sh) return fail(M4Q_E_UNSUPPORTED, "%s: no order-1 object for dim_x=%d dim_u=%d, which would hold the parameter-gradient kernels", who, dim_x, dim_u);
  if (B < 1 || N < 1) return fail(M4Q_E_BADARG, "%s: B and N must be at least 1 (got %d, %d)", who, B, N);
  if (!x0 || !u || !W || !data) return fail(M4Q_E_BADARG, "%s: x0, u, W and data are required", who);
  if (!dts || !op0 || !ops || !dirs) return fail(M4Q_E_BADARG, "%s: dts, op0, ops and dirs are required", who);
  if (!J || !grad_theta) return fail(M4Q_E_BADARG, "%s: J and grad_theta are required", who);
  if (int rc = check_plant_kind(who, /*named=*/true, plant_kind, dim_x, "parameter-gradient kernel",
                                "fit the parameters through its discretised model (m4q_discretize_batch, m4q_model_rollout_grad_batch)"))
    return rc;
  const int d = (int)plant_dim(plant_kind, dim_x);
  const int p_max = 16 / d - 1, p_tot = p + (grad_scale ? dim_u : 0);
  if (p < 1) return fail(M4Q_E_BADARG, "%s: p must be at least 1 (got %d)", who, p);
  if (p_tot > p_max)
    return fail(M4Q_E_UNSUPPORTED, "%s: %d directions (p = %d%s) are too many: the block matrix of (1 + p_tot) d columns must fit the 16 lanes "
                                   "of a row, at most %d directions for d = %d", who, p_tot, p, grad_scale ? " and the dim_u drive gains" : "",
                p_max, d);
  std::vector<double> cw((size_t)N + 1, 1.0);
  if (col_w)
    for (int32_t t = 0; t <= N; ++t) {
      if (!std::isfinite(col_w[t]) || col_w[t] < 0.0)
        return fail(M4Q_E_BADARG, "%s: col_w[%d] = %g is not a finite non-negative number", who, t, col_w[t]);
      cw[t] = col_w[t];
    }
  if (int rc = need_device()) return rc;
  const size_t n = dim_x, m = dim_u;
  const Extent ed(B, dirs_per_instance, (size_t)p * d * d), ey(B, data_per_instance, ((size_t)N + 1) * n);
  Stage st;
  m4q::ParamGradArgs a{};
  a.roll = stage_roll(st, B, n, m, N, x0, u, u_per_instance, u_scale, nullptr, nullptr, 0, /*xs_mode=*/2, /*xs=*/nullptr, /*q_mode=*/0, nullptr);
  a.roll.kind = plant_kind;
  a.roll.dts = st.in<double>(dts, N);
  a.roll.plant = stage_plant(st, B, plant_kind, dim_x, dim_u, op0, ops, plant_per_instance);
  a.roll.W = st.in<cplx>(W, n * n);
  a.p = p;
  a.dirs = st.in<cplx>(dirs, ed.count); a.dirs_stride = ed.stride;
  a.data = st.in<cplx>(data, ey.count); a.data_stride = ey.stride;
  a.col_w = st.in<double>(cw.data(), (size_t)N + 1);
  a.J = st.out<double>(J, (size_t)B);
  a.grad_theta = st.out<double>(grad_theta, (size_t)B * p);
  if (grad_scale) a.grad_scale = st.out<double>(grad_scale, (size_t)B * m);
  if (st.error()) return st.error();
  return st.finish(sh->launch_plant_param_grad(a, p_tot, nullptr), "plant parameter gradient");
}

int m4q_plant_linearize_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t plant_kind, int32_t T, const double* dts,
                              const double* X, const double* U, int32_t u_per_instance, const double* u_scale,
                              const double* op0, const double* ops, int32_t plant_per_instance,
                              double* A_ls, double* B_ls, double* Delta_ls) {
  const char* who = "m4q_plant_linearize_batch";
  const m4q::ShapeOps* sh = nullptr;
  if (int rc = plant_shape(who, /*named=*/false, dim_x, dim_u, /*needs_qp=*/false, &sh)) return rc;
  if (B < 1 || T < 1) return fail(M4Q_E_BADARG, "%s: B and T must be at least 1 (got %d, %d)", who, B, T);
  if ((int64_t)B * T > INT32_MAX) return fail(M4Q_E_BADARG, "%s: B T = %lld points do not fit one launch", who, (long long)B * T);
  if (!dts || !X || !U || !op0 || !ops) return fail(M4Q_E_BADARG, "%s: dts, X, U, op0 and ops are required", who);
  if (!A_ls && !B_ls && !Delta_ls) return fail(M4Q_E_BADARG, "%s: nothing to return (A_ls, B_ls and Delta_ls are all NULL)", who);
  if (int rc = check_plant_kind(who, /*named=*/false, plant_kind, dim_x, "linearisation kernel",
                                "linearise its discretised model with m4q_discretize_batch and m4q_linearize_batch"))
    return rc;
  if (int rc = need_device()) return rc;
  const size_t n = dim_x, m = dim_u, BT = (size_t)B * T;
  Stage st;
  m4q::PlantLinArgs a{};
  a.B = B; a.T = T; a.kind = plant_kind;
  a.traj = stage_traj(st, B, plant_kind, dim_x, dim_u, T, dts, X, U, u_per_instance, u_scale, op0, ops, plant_per_instance);
  if (A_ls) a.A_ls = st.out<cplx>(A_ls, BT * n * n);
  if (B_ls) a.B_ls = st.out<cplx>(B_ls, BT * n * m);
  if (Delta_ls) a.D_ls = st.out<cplx>(Delta_ls, BT * n);
  if (st.error()) return st.error();
  return st.finish(sh->launch_plant_linearize(a, nullptr), "plant linearize");
}

int m4q_plant_quad_program_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t plant_kind, int32_t T, const double* dts,
                                 const double* X, const double* U, int32_t u_per_instance, const double* u_scale,
                                 const double* op0, const double* ops, int32_t plant_per_instance,
                                 int32_t qp_flags, double sat, double du, const double* x_init, const double* X_bm,
                                 const double* U_bm, int32_t bm_per_instance, const double* Q_ls, const double* R_ls,
                                 const double* u_prev, double* X_opt, double* U_opt, double* cost, double* gains) {
  const char* who = "m4q_plant_quad_program_batch";
  // (the lookup admits plant-only shapes so that theirs is a refusal of its own: such an object holds no QP kernel)
  const m4q::ShapeOps* sh = nullptr;
  if (int rc = plant_shape(who, /*named=*/true, dim_x, dim_u, /*needs_qp=*/true, &sh)) return rc;
  if (B < 1 || T < 1) return fail(M4Q_E_BADARG, "%s: B and T must be at least 1 (got %d, %d)", who, B, T);
  if ((int64_t)B * T > INT32_MAX) return fail(M4Q_E_BADARG, "%s: B T = %lld points do not fit one launch", who, (long long)B * T);
  if (!dts || !X || !U || !op0 || !ops) return fail(M4Q_E_BADARG, "%s: dts, X, U, op0 and ops are required", who);
  if (!X_bm || !U_bm || !Q_ls || !R_ls || !X_opt || !U_opt || !cost)
    return fail(M4Q_E_BADARG, "%s: X_bm, U_bm, Q_ls, R_ls, X_opt, U_opt and cost are required", who);
  if (!(sat > 0)) return fail(M4Q_E_BADARG, "%s: sat must be positive", who);
  if (check_qp_flags(qp_flags)) {
    const std::string why = m4q_last_error();
    return fail(M4Q_E_BADARG, "%s: %s", who, why.c_str());
  }
  if (int rc = check_plant_kind(who, /*named=*/true, plant_kind, dim_x, "kernel here",
                                "use m4q_discretize_batch + m4q_linearize_batch + m4q_quad_program_batch"))
    return rc;
  const size_t n = dim_x, m = dim_u, k = plant_dim(plant_kind, dim_x), BT = (size_t)B * T, BT1 = (size_t)B * (T + 1);
  if ((qp_flags & M4Q_QP_EXACT_BOX) && (double)BT1 * n * 16 * 2 >= 4294967296.0)
    return fail(M4Q_E_BADARG, "%s: M4Q_QP_EXACT_BOX: batch too large for one call (trajectory workspace must stay below 4 GiB)", who);
  if (int rc = need_device()) return rc;
  const Extent xbm(B, bm_per_instance, (size_t)(T + 1) * n), ubm(B, bm_per_instance, (size_t)T * m);
  Stage st;
  m4q::PlantQpArgs a{};
  a.B = B; a.T = T; a.kind = plant_kind; a.flags = qp_flags; a.sat = sat; a.du = du;
  a.traj = stage_traj(st, B, plant_kind, dim_x, dim_u, T, dts, X, U, u_per_instance, u_scale, op0, ops, plant_per_instance);
  if (x_init) a.x_init = st.in<cplx>(x_init, (size_t)B * n);
  a.X_bm = st.in<cplx>(X_bm, xbm.count); a.xbm_stride = xbm.stride;
  a.U_bm = st.in<double>(U_bm, ubm.count); a.ubm_stride = ubm.stride;
  a.Q_ls = st.in<cplx>(Q_ls, (size_t)(T + 1) * n * n); a.R_ls = st.in<cplx>(R_ls, (size_t)T * m * m);
  if (u_prev) a.u_prev = st.in<double>(u_prev, (size_t)B * m);
  // the linearisation stays on the device: U_t (d x d, whatever the plant: k = d), B_t and Delta_t
  a.U_ws = st.out<cplx>(nullptr, BT * k * k); a.B_ws = st.out<cplx>(nullptr, BT * n * m); a.D_ws = st.out<cplx>(nullptr, BT * n);
  std::vector<int> sweeps;                                  // diagnostic (M4Q_QP_TRACE): pinned sweeps per instance
  if (qp_flags & M4Q_QP_EXACT_BOX) {
    if (getenv("M4Q_QP_TRACE")) {
      sweeps.resize(B);
      a.sweep_counts = st.out<int>(sweeps.data(), B);
    }
    a.X_alt = st.out<cplx>(nullptr, 2 * BT1 * n); a.U_alt = st.out<double>(nullptr, 2 * BT * m);
    a.pin_stat = st.out<double>(nullptr, BT * m);
  }
  a.X_opt = st.out<cplx>(X_opt, BT1 * n); a.U_opt = st.out<double>(U_opt, BT * m); a.cost = st.out<double>(cost, B);
  a.gains = st.out<cplx>(gains, BT * (n + 1) * m);          // (workspace when the caller wants no gains)
  if (st.error()) return st.error();
  const int rc = st.finish(sh->launch_plant_qp(a, nullptr), "plant qp");
  if (!rc && !sweeps.empty()) {
    long sum = 0;
    int mx = 0;
    for (int v : sweeps) { sum += v; mx = v > mx ? v : mx; }
    fprintf(stderr, "m4q: exact box QP on the plant: %d instances, pinned sweeps mean %.2f max %d\n", B, (double)sum / B, mx);
  }
  return rc;
}

// m4q_plant_sqp_batch and m4q_plant_ilqr_batch are one call - refusals, staging, launches - around one step launcher: closed
// says which candidates the step's line search runs (PlantStepArgs)
static int plant_descent_batch(const char* who, const char* what, int closed,
                               int32_t B, int32_t dim_x, int32_t dim_u, int32_t plant_kind, int32_t T, const double* dts,
                               const double* x0, const double* U0, int32_t u_per_instance, const double* u_scale,
                               const double* op0, const double* ops, int32_t plant_per_instance,
                               int32_t qp_flags, double sat, double du, const double* X_bm, const double* U_bm, int32_t bm_per_instance,
                               const double* Q_ls, const double* R_ls, const double* u_prev, int32_t iters, int32_t steps, double tol,
                               double* X, double* U, double* cost, double* cost_hist, double* alpha_hist, int32_t* n_iter, int32_t* status,
                               double* gains) {
  // the refusals of m4q_plant_quad_program_batch, whose launcher every iteration goes through, then the loop's own
  const m4q::ShapeOps* sh = nullptr;
  if (int rc = plant_shape(who, /*named=*/true, dim_x, dim_u, /*needs_qp=*/true, &sh)) return rc;
  if (B < 1 || T < 1) return fail(M4Q_E_BADARG, "%s: B and T must be at least 1 (got %d, %d)", who, B, T);
  if ((int64_t)B * T > INT32_MAX) return fail(M4Q_E_BADARG, "%s: B T = %lld points do not fit one launch", who, (long long)B * T);
  if (!x0 || !U0) return fail(M4Q_E_BADARG, "%s: x0 and U0, the initial states and the first guess, are required", who);
  if (!dts || !op0 || !ops) return fail(M4Q_E_BADARG, "%s: dts, op0 and ops are required", who);
  if (!X_bm || !U_bm || !Q_ls || !R_ls) return fail(M4Q_E_BADARG, "%s: X_bm, U_bm, Q_ls and R_ls are required", who);
  if (!X || !U || !cost || !cost_hist || !alpha_hist || !n_iter || !status)
    return fail(M4Q_E_BADARG, "%s: X, U, cost, cost_hist, alpha_hist, n_iter and status are required", who);
  if (!(sat > 0)) return fail(M4Q_E_BADARG, "%s: sat must be positive", who);
  if (check_qp_flags(qp_flags)) {
    const std::string why = m4q_last_error();
    return fail(M4Q_E_BADARG, "%s: %s", who, why.c_str());
  }
  if (iters < 1 || iters > 64) return fail(M4Q_E_BADARG, "%s: iters must be in 1..64, got %d", who, iters);
  if (steps < 1 || steps > 8) return fail(M4Q_E_BADARG, "%s: steps must be in 1..8, got %d", who, steps);
  if (!(tol >= 0) || !std::isfinite(tol)) return fail(M4Q_E_BADARG, "%s: tol must be finite and not negative", who);
  if (int rc = check_plant_kind(who, /*named=*/true, plant_kind, dim_x, "kernel here", "optimise on its discretised model")) return rc;
  const size_t n = dim_x, m = dim_u, k = plant_dim(plant_kind, dim_x), BT = (size_t)B * T, BT1 = (size_t)B * (T + 1);
  if ((qp_flags & M4Q_QP_EXACT_BOX) && (double)BT1 * n * 16 * 2 >= 4294967296.0)
    return fail(M4Q_E_BADARG, "%s: M4Q_QP_EXACT_BOX: batch too large for one call (trajectory workspace must stay below 4 GiB)", who);
  if (int rc = need_device()) return rc;
  const Extent eu(B, u_per_instance, (size_t)T * m);
  const Extent xbm(B, bm_per_instance, (size_t)(T + 1) * n), ubm(B, bm_per_instance, (size_t)T * m);
  Stage st;
  // staged once: the plant, the targets, the weights, x0 and U0; the iterate and every workspace live on the device
  m4q::PlantStepArgs s{};
  s.B = B; s.T = T; s.kind = plant_kind; s.flags = qp_flags; s.iters = iters; s.steps = steps; s.closed = closed; s.sat = sat; s.du = du; s.tol = tol;
  s.dts = st.in<double>(dts, T);
  s.x0 = st.in<cplx>(x0, (size_t)B * n);
  s.U0 = st.in<double>(U0, eu.count); s.u0_stride = eu.stride;
  if (u_scale) s.u_scale = st.in<double>(u_scale, (size_t)B * m);
  s.plant = stage_plant(st, B, plant_kind, dim_x, dim_u, op0, ops, plant_per_instance);
  s.X_bm = st.in<cplx>(X_bm, xbm.count); s.xbm_stride = xbm.stride;
  s.U_bm = st.in<double>(U_bm, ubm.count); s.ubm_stride = ubm.stride;
  s.Q_ls = st.in<cplx>(Q_ls, (size_t)(T + 1) * n * n); s.R_ls = st.in<cplx>(R_ls, (size_t)T * m * m);
  if (u_prev) s.u_prev = st.in<double>(u_prev, (size_t)B * m);
  s.X = st.out<cplx>(X, BT1 * n); s.U = st.out<double>(U, BT * m); s.cost = st.out<double>(cost, B);
  s.cost_hist = st.out<double>(cost_hist, (size_t)B * (iters + 1)); s.alpha_hist = st.out<double>(alpha_hist, (size_t)B * iters);
  s.n_iter = st.out<int>(n_iter, B); s.status = st.out<int>(status, B);
  s.X_lin = st.out<cplx>(nullptr, BT * n);
  double* U_qp = st.out<double>(nullptr, BT * m);
  s.U_qp = U_qp;
  // the QP of every iteration: m4q_plant_quad_program_batch's block on the iterate
  m4q::PlantQpArgs a{};
  a.B = B; a.T = T; a.kind = plant_kind; a.flags = qp_flags; a.sat = sat; a.du = du;
  a.traj.dts = s.dts; a.traj.X = s.X_lin; a.traj.U = s.U; a.traj.u_stride = (long)(T * m); a.traj.u_scale = s.u_scale;
  a.traj.plant = s.plant;
  a.x_init = s.x0; a.X_bm = s.X_bm; a.xbm_stride = s.xbm_stride; a.U_bm = s.U_bm; a.ubm_stride = s.ubm_stride;
  a.Q_ls = s.Q_ls; a.R_ls = s.R_ls; a.u_prev = s.u_prev;
  a.U_ws = st.out<cplx>(nullptr, BT * k * k); a.B_ws = st.out<cplx>(nullptr, BT * n * m); a.D_ws = st.out<cplx>(nullptr, BT * n);
  if (qp_flags & M4Q_QP_EXACT_BOX) {
    a.X_alt = st.out<cplx>(nullptr, 2 * BT1 * n); a.U_alt = st.out<double>(nullptr, 2 * BT * m);
    a.pin_stat = st.out<double>(nullptr, BT * m);
  }
  a.X_opt = st.out<cplx>(nullptr, BT1 * n); a.U_opt = U_qp; a.cost = st.out<double>(nullptr, B);
  a.gains = st.out<cplx>(gains, BT * (n + 1) * m);          // (workspace when the caller wants no gains)
  s.gains = a.gains;                                        // (the closed-loop step runs the law the QP just wrote)
  if (st.error()) return st.error();
  // one stream, no host synchronisation in between: the initial roll, then QP and step per iteration, then the gains' QP
  s.iter = -1;
  int rc = sh->launch_plant_step(s, nullptr);
  for (int i = 0; i < iters && !rc; ++i) {
    rc = sh->launch_plant_qp(a, nullptr);
    if (rc) break;
    s.iter = i;
    rc = sh->launch_plant_step(s, nullptr);
  }
  if (!rc && gains) rc = sh->launch_plant_qp(a, nullptr);
  return st.finish(rc, what);
}

int m4q_plant_sqp_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t plant_kind, int32_t T, const double* dts,
                        const double* x0, const double* U0, int32_t u_per_instance, const double* u_scale,
                        const double* op0, const double* ops, int32_t plant_per_instance,
                        int32_t qp_flags, double sat, double du, const double* X_bm, const double* U_bm, int32_t bm_per_instance,
                        const double* Q_ls, const double* R_ls, const double* u_prev, int32_t iters, int32_t steps, double tol,
                        double* X, double* U, double* cost, double* cost_hist, double* alpha_hist, int32_t* n_iter, int32_t* status,
                        double* gains) {
  return plant_descent_batch("m4q_plant_sqp_batch", "plant sqp", /*closed=*/0, B, dim_x, dim_u, plant_kind, T, dts, x0, U0, u_per_instance,
                             u_scale, op0, ops, plant_per_instance, qp_flags, sat, du, X_bm, U_bm, bm_per_instance, Q_ls, R_ls, u_prev, iters,
                             steps, tol, X, U, cost, cost_hist, alpha_hist, n_iter, status, gains);
}

int m4q_plant_ilqr_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t plant_kind, int32_t T, const double* dts,
                         const double* x0, const double* U0, int32_t u_per_instance, const double* u_scale,
                         const double* op0, const double* ops, int32_t plant_per_instance,
                         int32_t qp_flags, double sat, double du, const double* X_bm, const double* U_bm, int32_t bm_per_instance,
                         const double* Q_ls, const double* R_ls, const double* u_prev, int32_t iters, int32_t steps, double tol,
                         double* X, double* U, double* cost, double* cost_hist, double* alpha_hist, int32_t* n_iter, int32_t* status,
                         double* gains) {
  return plant_descent_batch("m4q_plant_ilqr_batch", "plant ilqr", /*closed=*/1, B, dim_x, dim_u, plant_kind, T, dts, x0, U0, u_per_instance,
                             u_scale, op0, ops, plant_per_instance, qp_flags, sat, du, X_bm, U_bm, bm_per_instance, Q_ls, R_ls, u_prev, iters,
                             steps, tol, X, U, cost, cost_hist, alpha_hist, n_iter, status, gains);
}

int m4q_model_rollout_grad_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t order, int32_t N, const double* x0, const double* u,
                                 int32_t u_per_instance, const double* u_scale, const double* models, int32_t model_per_instance,
                                 const double* W, const double* target, int32_t target_per_instance, int32_t q_mode,
                                 const double* weights, int32_t reduce, double* q, double* grad, double* grad_scale, double* q_mean) {
  const char* who = "m4q_model_rollout_grad_batch";
  const m4q::ShapeOps* sh = find_shape(dim_x, dim_u, order);
  if (!sh) return fail(M4Q_E_UNSUPPORTED, "no model kernel for dim_x=%d dim_u=%d order=%d", dim_x, dim_u, order);
  if (int rc = check_grad_args(who, B, N, x0, u, u_per_instance, W, target, q_mode, weights, reduce, q, grad, q_mean)) return rc;
  if (!models) return fail(M4Q_E_BADARG, "%s: models are required", who);
  if (int rc = need_device()) return rc;
  const size_t n = dim_x, m = dim_u, P = sh->np;
  const Extent mdl(B, model_per_instance, n * n * (1 + P));
  Stage st;
  m4q::GradArgs a = stage_grad(st, B, n, m, N, x0, u, u_per_instance, u_scale, W, target, target_per_instance, q_mode, weights, reduce, q,
                               grad, grad_scale, q_mean);
  a.roll.models = st.in<cplx>(models, mdl.count); a.roll.model_stride = mdl.stride;
  if (st.error()) return st.error();
  return st.finish(sh->launch_model_grad(a, nullptr), "model rollout gradient");
}

namespace {
// What m4q_plant_rollout_multi_batch and m4q_plant_robust_batch share: control sequences shared by the ensemble on one of the two
// unitary plants.  The refusals are those of m4q_plant_rollout_grad_batch with reduce set, in its order, checked before a device
// is asked for; *found receives the shape's kernels.
int check_ensemble_args(const char* who, int32_t B, int32_t dim_x, int32_t dim_u, int32_t plant_kind, int32_t N, const double* dts,
                        const double* x0, const double* u, const double* op0, const double* ops, const double* W, const double* target,
                        int32_t q_mode, const double* weights, const m4q::ShapeOps** found) {
  if (int rc = plant_shape(who, /*named=*/true, dim_x, dim_u, /*needs_qp=*/false, found)) return rc;
  if (B < 1 || N < 1) return fail(M4Q_E_BADARG, "%s: B and N must be at least 1 (got %d, %d)", who, B, N);
  if (!x0 || !u || !W || !target) return fail(M4Q_E_BADARG, "%s: x0, the control sequences, W and target are required", who);
  if (q_mode < 1 || q_mode > 2) return fail(M4Q_E_BADARG, "%s: q_mode is 1 (J = q_N) or 2 (J = sum_t q_t), got %d", who, q_mode);
  if (weights)
    for (int32_t b = 0; b < B; ++b)
      if (!std::isfinite(weights[b]) || weights[b] < 0.0) return fail(M4Q_E_BADARG, "%s: weights[%d] = %g is not a finite non-negative number", who, b, weights[b]);
  if (!dts || !op0 || !ops) return fail(M4Q_E_BADARG, "%s: dts, op0 and ops are required", who);
  // (the gradient's advice: the optimiser needs that gradient, and the kernels live in the other object)
  return check_plant_kind(who, /*named=*/true, plant_kind, dim_x, "kernel here",
                          "take the gradient of the discretised model with m4q_model_rollout_grad_batch");
}

// stages the ensemble once: the plant, x0, u_scale, W, the targets, dts, the weights (1 / B when absent), and the buffers of S
// sequences: us [S][N][m] (filled by the caller), J [B][S], the reduction's partials and F [S]
m4q::MultiArgs stage_ensemble(Stage& st, int32_t B, size_t n, size_t m, int32_t plant_kind, int32_t N, const double* dts, const double* x0,
                              const double* u_scale, const double* op0, const double* ops, int32_t plant_per_instance, const double* W,
                              const double* target, int32_t target_per_instance, int32_t q_mode, const double* weights, int32_t S) {
  const Extent ef(B, target_per_instance, n);
  m4q::MultiArgs a{};
  a.B = B; a.N = N; a.kind = plant_kind; a.S = S; a.q_mode = q_mode;
  a.dts = st.in<double>(dts, N);
  a.x0 = st.in<cplx>(x0, (size_t)B * n);
  if (u_scale) a.u_scale = st.in<double>(u_scale, (size_t)B * m);
  a.plant = stage_plant(st, B, plant_kind, (int32_t)n, (int32_t)m, op0, ops, plant_per_instance);
  a.W = st.in<cplx>(W, n * n);
  a.target = st.in<cplx>(target, ef.count); a.target_stride = ef.stride;
  std::vector<double> w;
  if (weights) w.assign(weights, weights + B);
  else w.assign((size_t)B, 1.0 / B);
  a.weights = st.in<double>(w.data(), (size_t)B);
  a.us = st.in<double>(nullptr, (size_t)S * N * m);
  a.J = st.out<double>(nullptr, (size_t)B * S);
  a.partial = st.out<double>(nullptr, (((size_t)B + m4q::GRAD_CHUNK - 1) / m4q::GRAD_CHUNK) * S);
  a.F = st.out<double>(nullptr, (size_t)S);
  return a;
}

int copy_up(const void* dev, const void* host, size_t bytes) {
  HIP_TRY(hipMemcpy(const_cast<void*>(dev), host, bytes, hipMemcpyHostToDevice));
  return 0;
}
int copy_down(void* host, const void* dev, size_t bytes) {
  HIP_TRY(hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost));
  return 0;
}
}  // namespace

int m4q_plant_rollout_multi_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t plant_kind, int32_t N, const double* dts,
                                  const double* x0, int32_t S, const double* us, const double* u_scale, const double* op0,
                                  const double* ops, int32_t plant_per_instance, const double* W, const double* target,
                                  int32_t target_per_instance, int32_t q_mode, const double* weights, double* J, double* F) {
  const char* who = "m4q_plant_rollout_multi_batch";
  const m4q::ShapeOps* sh = nullptr;
  if (int rc = check_ensemble_args(who, B, dim_x, dim_u, plant_kind, N, dts, x0, us, op0, ops, W, target, q_mode, weights, &sh)) return rc;
  if (S < 1 || S > m4q::MULTI_MAX_S) return fail(M4Q_E_BADARG, "%s: S must be in 1..%d, got %d", who, m4q::MULTI_MAX_S, S);
  if (!J && !F) return fail(M4Q_E_BADARG, "%s: nothing to return (J and F are both NULL)", who);
  if (int rc = need_device()) return rc;
  Stage st;
  m4q::MultiArgs a = stage_ensemble(st, B, dim_x, dim_u, plant_kind, N, dts, x0, u_scale, op0, ops, plant_per_instance, W, target,
                                    target_per_instance, q_mode, weights, S);
  if (st.error()) return st.error();
  const size_t nm = (size_t)N * dim_u;
  if (int rc = copy_up(a.us, us, (size_t)S * nm * sizeof(double))) return rc;
  if (!F) a.F = nullptr;                                     // (no reduction asked for)
  if (int rc = st.finish(sh->launch_plant_multi(a, nullptr), "plant multi rollout")) return rc;
  if (J)
    if (int rc = copy_down(J, a.J, (size_t)B * S * sizeof(double))) return rc;
  if (F)
    if (int rc = copy_down(F, a.F, (size_t)S * sizeof(double))) return rc;
  return 0;
}

namespace {
// What m4q_plant_robust_batch and m4q_model_robust_batch share behind their own ensemble checks: the refusals of the outputs and of
// the loop's parameters ...
// (the loop's parameters and its outputs, as both entries take them)
struct RobustParams {
  double sat; int32_t iters, steps, mem; double step0, tol, gtol;
};
struct RobustOut {
  double* U; double* cost; double* cost_hist; double* alpha_hist; double* pgrad_hist; int32_t* n_iter; int32_t* status; double* J;
};
int check_robust_args(const char* who, const RobustParams& p, const RobustOut& o) {
  const double sat = p.sat, step0 = p.step0, tol = p.tol, gtol = p.gtol;
  const int32_t iters = p.iters, steps = p.steps, mem = p.mem;
  const double *U = o.U, *cost = o.cost, *cost_hist = o.cost_hist, *alpha_hist = o.alpha_hist, *pgrad_hist = o.pgrad_hist;
  const int32_t *n_iter = o.n_iter, *status = o.status;
  if (!U || !cost || !cost_hist || !alpha_hist || !pgrad_hist || !n_iter || !status)
    return fail(M4Q_E_BADARG, "%s: U, cost, cost_hist, alpha_hist, pgrad_hist, n_iter and status are required", who);
  if (!(sat > 0)) return fail(M4Q_E_BADARG, "%s: sat must be positive (INFINITY: no box)", who);
  if (iters < 1 || iters > 64) return fail(M4Q_E_BADARG, "%s: iters must be in 1..64, got %d", who, iters);
  if (steps < 1 || steps > m4q::MULTI_MAX_S) return fail(M4Q_E_BADARG, "%s: steps must be in 1..%d, got %d", who, m4q::MULTI_MAX_S, steps);
  if (mem < 0 || mem > 8) return fail(M4Q_E_BADARG, "%s: mem must be in 0..8, got %d", who, mem);
  if (!(step0 > 0) || !std::isfinite(step0)) return fail(M4Q_E_BADARG, "%s: step0 must be positive and finite", who);
  if (!(tol >= 0) || !std::isfinite(tol) || !(gtol >= 0) || !std::isfinite(gtol))
    return fail(M4Q_E_BADARG, "%s: tol and gtol must be finite and not negative", who);
  return 0;
}

// ... and the loop itself (plant_robust.py: _loop is the definition; the direction is m4q_robust_host.h), written once on two
// launches: launch_grad(u) runs the reduced gradient at the sequence u [N][m] on the device and leaves the reduced gradient and F in
// d.mean [N m + 1]; launch_multi(us, S) rolls the S sequences at us and leaves J [B][S] in d.J and F [S] in d.F.  d.us is the
// candidates' buffer [steps][N m]: the iterate lives in the accepted candidate's slot of it.
struct RobustDev {
  const double* us; const double* mean; const double* F; const double* J;
};
int robust_loop(const char* who, int32_t B, size_t nm, const double* U0, const RobustParams& p, const RobustDev& d,
                const std::function<int(const double*)>& launch_grad, const std::function<int(const double*, int)>& launch_multi,
                const RobustOut& o) {
  const double sat = p.sat, step0 = p.step0, tol = p.tol, gtol = p.gtol;
  const int iters = p.iters, steps = p.steps, mem = p.mem;
  double *U = o.U, *cost = o.cost, *cost_hist = o.cost_hist, *alpha_hist = o.alpha_hist, *pgrad_hist = o.pgrad_hist, *J = o.J;
  int32_t *n_iter = o.n_iter, *status = o.status;
  m4q::robust::State r;
  r.mem = mem; r.sat = sat; r.step0 = step0;
  r.U.resize(nm);
  for (size_t e = 0; e < nm; ++e) r.U[e] = m4q::robust::clip(U0[e], sat);
  r.g.assign(nm, 0.0);
  std::vector<double> cands((size_t)steps * nm), down(nm + 1), Fs((size_t)steps);
  int slot = 0;                                               // where on the device the iterate is (-1: nowhere)
  if (int rc = copy_up(d.us, r.U.data(), nm * sizeof(double))) return rc;
  for (int i = 0; i <= iters; ++i) cost_hist[i] = 0.0;
  for (int i = 0; i < iters; ++i) alpha_hist[i] = pgrad_hist[i] = 0.0;
  double Fcur = 0.0;
  int st_code = 0, begun = 0;
  bool moved = true;
  for (int i = 0; i < iters; ++i) {
    if (moved) {                                              // step 1: the reduced gradient at the iterate, where it lies
      if (int rc = launch_grad(d.us + (size_t)slot * nm)) return fail(rc, "%s: gradient launch failed", who);
      if (int rc = copy_down(down.data(), d.mean, (nm + 1) * sizeof(double))) return rc;
      r.g.assign(down.begin(), down.begin() + nm);
      Fcur = down[nm];
      moved = false;
      if (i == 0) {
        for (int e = 0; e <= iters; ++e) cost_hist[e] = Fcur;
        if (!std::isfinite(Fcur)) { st_code = 3; break; }
      }
    }
    begun = i + 1;
    m4q::robust::project(r);                                  // steps 2 - 5 (m4q_robust_host.h)
    pgrad_hist[i] = r.gmax;
    if (r.gmax <= gtol) { st_code = 1; break; }
    m4q::robust::absorb(r);
    m4q::robust::direction(r);
    for (int j = 0; j < steps; ++j) m4q::robust::candidate(r, j, cands.data() + (size_t)j * nm);
    if (int rc = copy_up(d.us, cands.data(), cands.size() * sizeof(double))) return rc;
    slot = -1;
    if (int rc = launch_multi(d.us, steps)) return fail(rc, "%s: line search launch failed", who);
    if (int rc = copy_down(Fs.data(), d.F, Fs.size() * sizeof(double))) return rc;
    const int j = m4q::robust::pick(Fs.data(), steps);        // steps 6 - 8
    if (j >= 0 && Fs[j] < Fcur) {
      m4q::robust::accept(r, cands.data() + (size_t)j * nm);
      slot = j;
      moved = true;
      alpha_hist[i] = std::ldexp(1.0, -j);
      for (int e = i + 1; e <= iters; ++e) cost_hist[e] = Fs[j];
      const double dec = Fcur - Fs[j], Fold = Fcur;
      Fcur = Fs[j];
      if (dec <= tol * std::fabs(Fold)) { st_code = 1; break; }
    } else if (!r.pairs.empty()) {
      r.pairs.clear();
    } else {
      st_code = 2;
      break;
    }
  }
  for (size_t e = 0; e < nm; ++e) U[e] = r.U[e];
  cost[0] = Fcur; n_iter[0] = begun; status[0] = st_code;
  if (J) {                                                    // the members' objectives at the returned U: one S = 1 launch
    if (slot < 0) {
      if (int rc = copy_up(d.us, r.U.data(), nm * sizeof(double))) return rc;
      slot = 0;
    }
    if (int rc = launch_multi(d.us + (size_t)slot * nm, 1)) return fail(rc, "%s: final launch failed", who);
    double Fone = 0.0;
    if (int rc = copy_down(J, d.J, (size_t)B * sizeof(double))) return rc;
    if (int rc = copy_down(&Fone, d.F, sizeof(double))) return rc;
    if (std::isfinite(Fcur) && Fone != Fcur)
      return fail(-(int)hipErrorUnknown, "%s: the mean of the members' objectives at U, %.17g, is not the cost %.17g", who, Fone, Fcur);
  }
  HIP_TRY(hipDeviceSynchronize());
  return 0;
}
}  // namespace

int m4q_plant_robust_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t plant_kind, int32_t N, const double* dts, const double* x0,
                           const double* U0, const double* u_scale, const double* op0, const double* ops, int32_t plant_per_instance,
                           const double* W, const double* target, int32_t target_per_instance, int32_t q_mode, const double* weights,
                           double sat, int32_t iters, int32_t steps, int32_t mem, double step0, double tol, double gtol,
                           double* U, double* cost, double* cost_hist, double* alpha_hist, double* pgrad_hist, int32_t* n_iter,
                           int32_t* status, double* J) {
  const char* who = "m4q_plant_robust_batch";
  const m4q::ShapeOps* sh = nullptr;
  if (int rc = check_ensemble_args(who, B, dim_x, dim_u, plant_kind, N, dts, x0, U0, op0, ops, W, target, q_mode, weights, &sh)) return rc;
  const RobustParams prm{sat, iters, steps, mem, step0, tol, gtol};
  const RobustOut out{U, cost, cost_hist, alpha_hist, pgrad_hist, n_iter, status, J};
  if (int rc = check_robust_args(who, prm, out)) return rc;
  if (int rc = need_device()) return rc;
  const size_t n = dim_x, m = dim_u, nm = (size_t)N * m;
  // staged once: the ensemble and every workspace; the iterate lives in a slot of the candidates' buffer
  Stage st;
  m4q::MultiArgs c = stage_ensemble(st, B, n, m, plant_kind, N, dts, x0, u_scale, op0, ops, plant_per_instance, W, target,
                                    target_per_instance, q_mode, weights, steps);
  m4q::GradArgs g{};
  g.roll.B = B; g.roll.N = N; g.roll.kind = plant_kind; g.roll.xs_mode = 2; g.roll.q_mode = q_mode;
  g.roll.dts = c.dts; g.roll.x0 = c.x0; g.roll.u_scale = c.u_scale; g.roll.u_stride = 0;
  g.roll.plant = c.plant;
  g.roll.W = c.W; g.roll.target = c.target; g.roll.target_stride = c.target_stride;
  g.roll.xs = st.out<cplx>(nullptr, (size_t)B * ((size_t)N + 1) * n);
  g.roll.q = st.out<double>(nullptr, (size_t)B * (q_mode == 2 ? (size_t)N + 1 : 1));
  g.grad = st.out<double>(nullptr, (size_t)B * nm);
  g.reduce = 1;
  g.weights = c.weights;
  g.partial = st.out<double>(nullptr, (((size_t)B + m4q::GRAD_CHUNK - 1) / m4q::GRAD_CHUNK) * (nm + 1));
  double* mean = st.out<double>(nullptr, nm + 1);             // the reduced gradient [N][m], then F: one copy down per gradient
  g.grad_mean = mean; g.q_mean = mean + nm;
  if (st.error()) return st.error();

  const RobustDev d{c.us, mean, c.F, c.J};
  return robust_loop(
      who, B, nm, U0, prm, d,
      [&](const double* u) { g.roll.u = u; return sh->launch_plant_grad(g, nullptr); },
      [&](const double* us, int S) { m4q::MultiArgs one = c; one.S = S; one.us = us; return sh->launch_plant_multi(one, nullptr); },
      out);
}

namespace {
// What m4q_model_rollout_multi_batch and m4q_model_robust_batch share: control sequences shared by the ensemble on the members'
// models.  The refusals are those of m4q_model_rollout_grad_batch with reduce set, in its order and under the entry's name, checked
// before a device is asked for; *found receives the shape's kernels.
int check_model_ensemble_args(const char* who, int32_t B, int32_t dim_x, int32_t dim_u, int32_t order, int32_t N, const double* x0,
                              const double* u, const double* models, const double* W, const double* target, int32_t q_mode,
                              const double* weights, const m4q::ShapeOps** found) {
  *found = find_shape(dim_x, dim_u, order);
  if (!*found) return fail(M4Q_E_UNSUPPORTED, "%s: no model kernel for dim_x=%d dim_u=%d order=%d", who, dim_x, dim_u, order);
  if (B < 1 || N < 1) return fail(M4Q_E_BADARG, "%s: B and N must be at least 1 (got %d, %d)", who, B, N);
  if (!x0 || !u || !W || !target) return fail(M4Q_E_BADARG, "%s: x0, the control sequences, W and target are required", who);
  if (q_mode < 1 || q_mode > 2) return fail(M4Q_E_BADARG, "%s: q_mode is 1 (J = q_N) or 2 (J = sum_t q_t), got %d", who, q_mode);
  if (weights)
    for (int32_t b = 0; b < B; ++b)
      if (!std::isfinite(weights[b]) || weights[b] < 0.0) return fail(M4Q_E_BADARG, "%s: weights[%d] = %g is not a finite non-negative number", who, b, weights[b]);
  if (!models) return fail(M4Q_E_BADARG, "%s: models are required", who);
  return 0;
}

// stage_ensemble for models: the models, x0, u_scale, W, the targets, the weights (1 / B when absent), and the buffers of S sequences
m4q::ModelMultiArgs stage_model_ensemble(Stage& st, int32_t B, size_t n, size_t m, size_t P, int32_t N, const double* x0,
                                         const double* u_scale, const double* models, int32_t model_per_instance, const double* W,
                                         const double* target, int32_t target_per_instance, int32_t q_mode, const double* weights, int32_t S) {
  const Extent ef(B, target_per_instance, n), mdl(B, model_per_instance, n * n * (1 + P));
  m4q::ModelMultiArgs a{};
  a.B = B; a.N = N; a.S = S; a.q_mode = q_mode;
  a.x0 = st.in<cplx>(x0, (size_t)B * n);
  if (u_scale) a.u_scale = st.in<double>(u_scale, (size_t)B * m);
  a.models = st.in<cplx>(models, mdl.count); a.model_stride = mdl.stride;
  a.W = st.in<cplx>(W, n * n);
  a.target = st.in<cplx>(target, ef.count); a.target_stride = ef.stride;
  std::vector<double> w;
  if (weights) w.assign(weights, weights + B);
  else w.assign((size_t)B, 1.0 / B);
  a.weights = st.in<double>(w.data(), (size_t)B);
  a.us = st.in<double>(nullptr, (size_t)S * N * m);
  a.J = st.out<double>(nullptr, (size_t)B * S);
  a.partial = st.out<double>(nullptr, (((size_t)B + m4q::GRAD_CHUNK - 1) / m4q::GRAD_CHUNK) * S);
  a.F = st.out<double>(nullptr, (size_t)S);
  return a;
}
}  // namespace

int m4q_model_rollout_multi_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t order, int32_t N, const double* x0, int32_t S,
                                  const double* us, const double* u_scale, const double* models, int32_t model_per_instance,
                                  const double* W, const double* target, int32_t target_per_instance, int32_t q_mode,
                                  const double* weights, double* J, double* F) {
  const char* who = "m4q_model_rollout_multi_batch";
  const m4q::ShapeOps* sh = nullptr;
  if (int rc = check_model_ensemble_args(who, B, dim_x, dim_u, order, N, x0, us, models, W, target, q_mode, weights, &sh)) return rc;
  if (S < 1 || S > m4q::MULTI_MAX_S) return fail(M4Q_E_BADARG, "%s: S must be in 1..%d, got %d", who, m4q::MULTI_MAX_S, S);
  if (!J && !F) return fail(M4Q_E_BADARG, "%s: nothing to return (J and F are both NULL)", who);
  if (int rc = need_device()) return rc;
  Stage st;
  m4q::ModelMultiArgs a = stage_model_ensemble(st, B, dim_x, dim_u, sh->np, N, x0, u_scale, models, model_per_instance, W, target,
                                               target_per_instance, q_mode, weights, S);
  if (st.error()) return st.error();
  const size_t nm = (size_t)N * dim_u;
  if (int rc = copy_up(a.us, us, (size_t)S * nm * sizeof(double))) return rc;
  if (!F) a.F = nullptr;                                     // (no reduction asked for)
  if (int rc = st.finish(sh->launch_model_multi(a, nullptr), "model multi rollout")) return rc;
  if (J)
    if (int rc = copy_down(J, a.J, (size_t)B * S * sizeof(double))) return rc;
  if (F)
    if (int rc = copy_down(F, a.F, (size_t)S * sizeof(double))) return rc;
  return 0;
}

int m4q_model_robust_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t order, int32_t N, const double* x0, const double* U0,
                           const double* u_scale, const double* models, int32_t model_per_instance, const double* W,
                           const double* target, int32_t target_per_instance, int32_t q_mode, const double* weights,
                           double sat, int32_t iters, int32_t steps, int32_t mem, double step0, double tol, double gtol,
                           double* U, double* cost, double* cost_hist, double* alpha_hist, double* pgrad_hist, int32_t* n_iter,
                           int32_t* status, double* J) {
  const char* who = "m4q_model_robust_batch";
  const m4q::ShapeOps* sh = nullptr;
  if (int rc = check_model_ensemble_args(who, B, dim_x, dim_u, order, N, x0, U0, models, W, target, q_mode, weights, &sh)) return rc;
  const RobustParams prm{sat, iters, steps, mem, step0, tol, gtol};
  const RobustOut out{U, cost, cost_hist, alpha_hist, pgrad_hist, n_iter, status, J};
  if (int rc = check_robust_args(who, prm, out)) return rc;
  if (int rc = need_device()) return rc;
  const size_t n = dim_x, m = dim_u, nm = (size_t)N * m;
  // staged once: the ensemble and every workspace; the iterate lives in a slot of the candidates' buffer
  Stage st;
  m4q::ModelMultiArgs c = stage_model_ensemble(st, B, n, m, sh->np, N, x0, u_scale, models, model_per_instance, W, target,
                                               target_per_instance, q_mode, weights, steps);
  m4q::GradArgs g{};
  g.roll.B = B; g.roll.N = N; g.roll.xs_mode = 2; g.roll.q_mode = q_mode;
  g.roll.x0 = c.x0; g.roll.u_scale = c.u_scale; g.roll.u_stride = 0;
  g.roll.models = c.models; g.roll.model_stride = c.model_stride;
  g.roll.W = c.W; g.roll.target = c.target; g.roll.target_stride = c.target_stride;
  g.roll.xs = st.out<cplx>(nullptr, (size_t)B * ((size_t)N + 1) * n);
  g.roll.q = st.out<double>(nullptr, (size_t)B * (q_mode == 2 ? (size_t)N + 1 : 1));
  g.grad = st.out<double>(nullptr, (size_t)B * nm);
  g.reduce = 1;
  g.weights = c.weights;
  g.partial = st.out<double>(nullptr, (((size_t)B + m4q::GRAD_CHUNK - 1) / m4q::GRAD_CHUNK) * (nm + 1));
  double* mean = st.out<double>(nullptr, nm + 1);             // the reduced gradient [N][m], then F: one copy down per gradient
  g.grad_mean = mean; g.q_mean = mean + nm;
  if (st.error()) return st.error();

  const RobustDev d{c.us, mean, c.F, c.J};
  return robust_loop(
      who, B, nm, U0, prm, d,
      [&](const double* u) { g.roll.u = u; return sh->launch_model_grad(g, nullptr); },
      [&](const double* us, int S) { m4q::ModelMultiArgs one = c; one.S = S; one.us = us; return sh->launch_model_multi(one, nullptr); },
      out);
}

// what the fit against a prior model adds to the fit's arguments (m4q_dmdc_refit_batch, m4q_dmdc_refit_qr_batch)
struct PriorIn {
  const double* A0; int32_t A0_per_instance;
  const double* discount; int32_t discount_per_instance;
  const int32_t* counts;
};

// the two routes of the DMDc fit share their arguments, their checks and their staging: qr names the QR route's entry points;
// prior: the fit against a prior model (the refit entry points), null for the plain fit
static int dmdc_fit(const char* who, bool qr, int32_t B, int32_t dim_x, int32_t dim_u, int32_t order, int32_t E, int32_t N, const double* xs,
                    const double* u, int32_t u_per_instance, const double* u_scale, const double* rconds, int32_t R, double* models,
                    int32_t* ranks, double* svals, int32_t* status, const PriorIn* prior = nullptr) {
  const m4q::ShapeOps* sh = find_shape(dim_x, dim_u, order);
  if (!sh) return fail(M4Q_E_UNSUPPORTED, "no model kernel for dim_x=%d dim_u=%d order=%d", dim_x, dim_u, order);
  if (sh->fit_lds_bytes == 0)
    return fail(M4Q_E_UNSUPPORTED, "%s: the %s data of dim_x=%d dim_u=%d order=%d (nz = %d) do not fit one workgroup's "
                "LDS; fit such models on the host (DiscrepDMDc.from_data)", who, qr ? "factored" : "Gram", dim_x, dim_u, order,
                dim_x * (1 + sh->np));
  if (B < 1 || E < 1 || N < 1) return fail(M4Q_E_BADARG, "%s: B, E and N must be at least 1 (got %d, %d, %d)", who, B, E, N);
  if (R < 1 || R > M4Q_FIT_MAX_RCONDS) return fail(M4Q_E_BADARG, "%s: R must be 1..%d, got %d", who, M4Q_FIT_MAX_RCONDS, R);
  if (!xs || !u || !rconds || !models || !status) return fail(M4Q_E_BADARG, "%s: xs, u, rconds, models and status are required", who);
  const double rcond_min = qr ? M4Q_FIT_QR_RCOND_MIN : M4Q_FIT_RCOND_MIN;
  for (int r = 0; r < R; ++r)
    if (!(rconds[r] >= rcond_min && rconds[r] < 1.0))
      return fail(M4Q_E_BADARG, "%s: rconds[%d] = %g is outside [%g, 1): below that the cut-off lies in the %s "
                  "(fit on the host with DiscrepDMDc.from_data)", who, r, rconds[r], rcond_min,
                  qr ? "rounding of the data themselves" : "Gram matrix's rounding floor");
  if (prior) {
    if (!prior->A0 || !prior->discount) return fail(M4Q_E_BADARG, "%s: A0 and discount are required", who);
    for (int b = 0; b < (prior->discount_per_instance ? B : 1); ++b)
      if (!(prior->discount[b] > 0.0 && prior->discount[b] <= 1.0))
        return fail(M4Q_E_BADARG, "%s: discount[%d] = %g is outside (0, 1]", who, b, prior->discount[b]);
    if (prior->counts)
      for (int b = 0; b < B; ++b)
        if (prior->counts[b] < 0 || prior->counts[b] > N)
          return fail(M4Q_E_BADARG, "%s: counts[%d] = %d is outside [0, N = %d]", who, b, prior->counts[b], N);
  }
  if (int rc = need_device()) return rc;
  const size_t n = dim_x, m = dim_u, nz = n * (1 + (size_t)sh->np);
  const Extent eu(B, u_per_instance, (size_t)E * N * m);
  Stage st;
  m4q::RefitArgs ra{};
  m4q::FitArgs& a = ra.fit;
  a.B = B; a.E = E; a.N = N; a.R = R;
  a.xs = st.in<cplx>(xs, (size_t)B * E * ((size_t)N + 1) * n);
  a.u = st.in<double>(u, eu.count); a.u_stride = eu.stride;
  if (u_scale) a.u_scale = st.in<double>(u_scale, (size_t)B * m);
  a.rconds = st.in<double>(rconds, R);
  a.models = st.out<cplx>(models, (size_t)R * B * n * nz);
  if (ranks) a.ranks = st.out<int>(ranks, (size_t)R * B);
  if (svals) a.svals = st.out<double>(svals, (size_t)B * nz);
  a.status = st.out<int>(status, B);
  if (prior) {
    const Extent ea(B, prior->A0_per_instance, n * nz), ed(B, prior->discount_per_instance, 1);
    ra.A0 = st.in<cplx>(prior->A0, ea.count); ra.A0_stride = ea.stride;
    ra.discount = st.in<double>(prior->discount, ed.count); ra.discount_stride = ed.stride;
    if (prior->counts) ra.counts = st.in<int>(prior->counts, B);
  }
  if (st.error()) return st.error();
  if (prior)
    return qr ? st.finish(sh->launch_refit_qr(ra, nullptr), "DMDc fit against a prior (QR)")
              : st.finish(sh->launch_refit(ra, nullptr), "DMDc fit against a prior");
  return qr ? st.finish(sh->launch_fit_qr(a, nullptr), "DMDc fit (QR)") : st.finish(sh->launch_fit(a, nullptr), "DMDc fit");
}

int m4q_dmdc_fit_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t order, int32_t E, int32_t N, const double* xs, const double* u,
                       int32_t u_per_instance, const double* u_scale, const double* rconds, int32_t R, double* models, int32_t* ranks,
                       double* svals, int32_t* status) {
  return dmdc_fit("m4q_dmdc_fit_batch", false, B, dim_x, dim_u, order, E, N, xs, u, u_per_instance, u_scale, rconds, R, models, ranks, svals,
                  status);
}

int m4q_dmdc_fit_qr_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t order, int32_t E, int32_t N, const double* xs, const double* u,
                          int32_t u_per_instance, const double* u_scale, const double* rconds, int32_t R, double* models, int32_t* ranks,
                          double* svals, int32_t* status) {
  return dmdc_fit("m4q_dmdc_fit_qr_batch", true, B, dim_x, dim_u, order, E, N, xs, u, u_per_instance, u_scale, rconds, R, models, ranks,
                  svals, status);
}

int m4q_dmdc_refit_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t order, int32_t E, int32_t N, const double* xs, const double* u,
                         int32_t u_per_instance, const double* u_scale, const double* rconds, int32_t R, double* models, int32_t* ranks,
                         double* svals, int32_t* status, const double* A0, int32_t A0_per_instance, const double* discount,
                         int32_t discount_per_instance, const int32_t* counts) {
  const PriorIn prior{A0, A0_per_instance, discount, discount_per_instance, counts};
  return dmdc_fit("m4q_dmdc_refit_batch", false, B, dim_x, dim_u, order, E, N, xs, u, u_per_instance, u_scale, rconds, R, models, ranks,
                  svals, status, &prior);
}

int m4q_dmdc_refit_qr_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t order, int32_t E, int32_t N, const double* xs, const double* u,
                            int32_t u_per_instance, const double* u_scale, const double* rconds, int32_t R, double* models, int32_t* ranks,
                            double* svals, int32_t* status, const double* A0, int32_t A0_per_instance, const double* discount,
                            int32_t discount_per_instance, const int32_t* counts) {
  const PriorIn prior{A0, A0_per_instance, discount, discount_per_instance, counts};
  return dmdc_fit("m4q_dmdc_refit_qr_batch", true, B, dim_x, dim_u, order, E, N, xs, u, u_per_instance, u_scale, rconds, R, models,
                  ranks, svals, status, &prior);
}

int m4q_online_dmdc_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t order, int32_t E, int32_t N, const double* xs, const double* u,
                          int32_t u_per_instance, const double* u_scale, const int32_t* counts, const double* A0, int32_t A0_per_instance,
                          const double* P0, int32_t P0_per_instance, double alpha, const double* discount, int32_t discount_per_instance,
                          int32_t flags, int32_t hist_every, double* models, double* P, double* hist, double* innov, int32_t* status) {
  const m4q::ShapeOps* sh = find_shape(dim_x, dim_u, order);
  if (!sh) return fail(M4Q_E_UNSUPPORTED, "no model kernel for dim_x=%d dim_u=%d order=%d", dim_x, dim_u, order);
  if (sh->online_lds_bytes == 0)
    return fail(M4Q_E_UNSUPPORTED, "m4q_online_dmdc_batch: the state of dim_x=%d dim_u=%d order=%d (nz = %d) does not fit one wavefront "
                "and one workgroup's LDS; update such models on the host (OnlineDMDc.fit_iteration)", dim_x, dim_u, order,
                dim_x * (1 + sh->np));
  if (B < 1 || E < 1 || N < 1) return fail(M4Q_E_BADARG, "m4q_online_dmdc_batch: B, E and N must be at least 1 (got %d, %d, %d)", B, E, N);
  if (hist_every < 0) return fail(M4Q_E_BADARG, "m4q_online_dmdc_batch: hist_every must not be negative, got %d", hist_every);
  if (flags & ~M4Q_ONLINE_HERMITIAN) return fail(M4Q_E_BADARG, "m4q_online_dmdc_batch: flags has bits outside M4Q_ONLINE_HERMITIAN (0x%x)", flags);
  if (!xs || !u || !A0 || !discount || !models || !status)
    return fail(M4Q_E_BADARG, "m4q_online_dmdc_batch: xs, u, A0, discount, models and status are required");
  if (!P0 && !(alpha > 0.0 && alpha <= DBL_MAX))
    return fail(M4Q_E_BADARG, "m4q_online_dmdc_batch: without P0, alpha must be positive and finite (P0 = alpha I), got %g", alpha);
  for (int b = 0; b < (discount_per_instance ? B : 1); ++b)
    if (!(discount[b] > 0.0 && discount[b] <= 1.0))
      return fail(M4Q_E_BADARG, "m4q_online_dmdc_batch: discount[%d] = %g is outside (0, 1]", b, discount[b]);
  if (counts)
    for (int b = 0; b < B; ++b)
      if (counts[b] < 0 || counts[b] > N)
        return fail(M4Q_E_BADARG, "m4q_online_dmdc_batch: counts[%d] = %d is outside [0, N = %d]", b, counts[b], N);
  if (int rc = need_device()) return rc;
  const size_t n = dim_x, m = dim_u, nz = n * (1 + (size_t)sh->np);
  const Extent eu(B, u_per_instance, (size_t)E * N * m), ea(B, A0_per_instance, n * nz), ep(B, P0_per_instance, nz * nz),
      ed(B, discount_per_instance, 1);
  Stage st;
  m4q::OnlineArgs a{};
  a.B = B; a.E = E; a.N = N; a.alpha = alpha;
  a.xs = st.in<cplx>(xs, (size_t)B * E * ((size_t)N + 1) * n);
  a.u = st.in<double>(u, eu.count); a.u_stride = eu.stride;
  if (u_scale) a.u_scale = st.in<double>(u_scale, (size_t)B * m);
  if (counts) a.counts = st.in<int>(counts, B);
  a.A0 = st.in<cplx>(A0, ea.count); a.A0_stride = ea.stride;
  if (P0) { a.P0 = st.in<cplx>(P0, ep.count); a.P0_stride = ep.stride; }
  a.discount = st.in<double>(discount, ed.count); a.discount_stride = ed.stride;
  a.models = st.out<cplx>(models, (size_t)B * n * nz);
  if (P) a.P = st.out<cplx>(P, (size_t)B * nz * nz);
  const size_t H = hist_every > 0 ? ((size_t)E * N) / hist_every : 0;
  if (hist && H > 0) { a.hist_every = hist_every; a.hist = st.out<cplx>(hist, H * B * n * nz); }
  if (innov) a.innov = st.out<double>(innov, (size_t)B * E * N);
  a.status = st.out<int>(status, B);
  if (st.error()) return st.error();
  return st.finish(sh->launch_online(a, (flags & M4Q_ONLINE_HERMITIAN) != 0, nullptr), "online DMDc");
}

int m4q_mpc_batch(const m4q_problem* p, int32_t B, const double* models, const double* x0, const double* X_targ,
                  const double* U_targ, const double* Q, const double* R, const double* Qf, const double* op0,
                  const double* ops, double* xs, double* us, int32_t* exit_codes, int32_t* steps_done,
                  int32_t* qp_solves) {
  if (!p || !models || !x0 || !X_targ || !U_targ || !Q || !R || !Qf || !xs || !us)
    return fail(M4Q_E_BADARG, "m4q_mpc_batch: bad argument");
  if (p->plant_kind == M4Q_PLANT_NONE) return fail(M4Q_E_BADARG, "m4q_mpc_batch needs a device plant; use the session API for host plants");
  if (!op0 || !ops) return fail(M4Q_E_BADARG, "m4q_mpc_batch: plant operators missing");
  m4q_session* s = nullptr;
  int rc = m4q_session_create(p, B, -1, &s);
  if (rc) return rc;
  struct Guard { m4q_session* s; ~Guard() { m4q_session_destroy(s); } } guard{s};
  const void* in[9] = {models, x0, X_targ, U_targ, Q, R, Qf, op0, ops};
  for (int f = M4Q_F_MODELS; f <= M4Q_F_OPS; ++f)
    if ((rc = m4q_session_upload(s, f, in[f], s->fbytes[f]))) return rc;
  if ((rc = m4q_session_run(s, 0, p->n_steps))) return rc;
  if ((rc = m4q_session_sync(s))) return rc;
  if ((rc = m4q_session_download(s, M4Q_F_XS, xs, s->fbytes[M4Q_F_XS]))) return rc;
  if ((rc = m4q_session_download(s, M4Q_F_US, us, s->fbytes[M4Q_F_US]))) return rc;
  if (exit_codes && (rc = m4q_session_download(s, M4Q_F_CODES, exit_codes, s->fbytes[M4Q_F_CODES]))) return rc;
  if (steps_done && (rc = m4q_session_download(s, M4Q_F_STEPS_DONE, steps_done, s->fbytes[M4Q_F_STEPS_DONE]))) return rc;
  if (qp_solves && (rc = m4q_session_download(s, M4Q_F_QP_SOLVES, qp_solves, s->fbytes[M4Q_F_QP_SOLVES]))) return rc;
  return 0;
}

int m4q_session_copy_final_state(m4q_session* s, void* dst_dev) {
  if (!s || !dst_dev) return fail(M4Q_E_BADARG, "m4q_session_copy_final_state: bad argument");
  const size_t row = (size_t)s->prob.dim_x * 16;
  HIP_TRY(hipMemcpy2DAsync(dst_dev, row, (const char*)s->f[M4Q_F_XS].p + (size_t)s->prob.n_steps * row,
                           (size_t)(s->prob.n_steps + 1) * row, row, s->B, hipMemcpyDeviceToDevice, s->stream));
  return 0;
}

// the watchdog flag of the launches queued so far, as one int32 in caller-owned device memory (a gather buffer's status word:
// rank dst learns from the gathered bytes that some rank's launch abandoned itself); enqueued on the session stream
int m4q_session_copy_status(m4q_session* s, void* dst_dev) {
  if (!s || !dst_dev) return fail(M4Q_E_BADARG, "m4q_session_copy_status: bad argument");
  HIP_TRY(hipMemcpyAsync(dst_dev, (const char*)s->queue.p + 4, 4, hipMemcpyDeviceToDevice, s->stream));
  return 0;
}

// ------------------------------------------------------------------------------------------
// communicator: RCCL through dlopen (no link-time dependency), its own stream, one event per gather slot
// ------------------------------------------------------------------------------------------
namespace {
struct Rccl {
  void* h = nullptr;
  decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
  decltype(&ncclCommInitRank) CommInitRank = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclGather) Gather = nullptr;
  decltype(&ncclAllReduce) AllReduce = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
  std::string why;
};
Rccl* rccl() {
  static Rccl r;
  static bool tried = false;
  if (tried) return &r;
  tried = true;
  const char* env = std::getenv("M4Q_RCCL_LIB");
  const char* names[] = {env, "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"};
  for (const char* n : names) {
    if (!n || !*n) continue;
    r.h = dlopen(n, RTLD_NOW | RTLD_LOCAL);
    if (r.h) break;
    const char* e = dlerror();          // NULL when no error is pending: never into a std::string as it is
    r.why = e ? e : "dlopen failed (no dlerror text)";
  }
  if (!r.h) return &r;
  bool ok = true;
  auto sym = [&](const char* n) { void* p = dlsym(r.h, n); if (!p) { ok = false; r.why = std::string("missing symbol ") + n; } return p; };
  r.GetUniqueId = (decltype(r.GetUniqueId))sym("ncclGetUniqueId");
  r.CommInitRank = (decltype(r.CommInitRank))sym("ncclCommInitRank");
  r.CommDestroy = (decltype(r.CommDestroy))sym("ncclCommDestroy");
  r.Gather = (decltype(r.Gather))sym("ncclGather");
  r.AllReduce = (decltype(r.AllReduce))sym("ncclAllReduce");
  r.GetErrorString = (decltype(r.GetErrorString))sym("ncclGetErrorString");
  if (!ok) { dlclose(r.h); r.h = nullptr; }
  return &r;
}
int need_rccl(Rccl** out) {
  Rccl* r = rccl();
  if (!r->h) return fail(M4Q_E_COMM, "librccl.so could not be loaded (%s); set M4Q_RCCL_LIB", r->why.c_str());
  *out = r;
  return 0;
}
#define NCCL_TRY(r, expr)                                                                     \
  do {                                                                                         \
    ncclResult_t e_ = (expr);                                                                  \
    if (e_ != ncclSuccess) return fail(M4Q_E_COMM, "%s: %s", #expr, (r)->GetErrorString(e_)); \
  } while (0)
}  // namespace

struct m4q_comm {
  ncclComm_t comm = nullptr;
  int rank = 0, world = 1, device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t slot[8] = {};
  hipEvent_t dep = nullptr;
  double* scratch = nullptr;        // 64 doubles in, 64 out (m4q_comm_allreduce_f64)
};

int m4q_comm_unique_id(void* id128) {
  static_assert(sizeof(ncclUniqueId) == M4Q_UNIQUE_ID_BYTES, "unique id size");
  if (!id128) return fail(M4Q_E_BADARG, "m4q_comm_unique_id: null buffer");
  Rccl* r;
  int rc = need_rccl(&r);
  if (rc) return rc;
  ncclUniqueId id;
  NCCL_TRY(r, r->GetUniqueId(&id));
  std::memcpy(id128, &id, sizeof(id));
  return 0;
}

int m4q_comm_create(int32_t rank, int32_t world, const void* id128, int32_t device, m4q_comm** out) {
  if (!out || !id128 || world < 1 || rank < 0 || rank >= world) return fail(M4Q_E_BADARG, "m4q_comm_create: bad argument");
  int rc = need_device();
  if (rc) return rc;
  Rccl* r;
  if ((rc = need_rccl(&r))) return rc;
  if (device >= 0) HIP_TRY(hipSetDevice(device));
  m4q_comm* c = new m4q_comm();
  c->rank = rank;
  c->world = world;
  struct Guard { m4q_comm* c; ~Guard() { if (c) m4q_comm_destroy(c); } } guard{c};
  HIP_TRY(hipGetDevice(&c->device));
  HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  for (auto& e : c->slot) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&c->dep, hipEventDisableTiming));
  HIP_TRY(hipMalloc((void**)&c->scratch, 128 * sizeof(double)));
  ncclUniqueId id;
  std::memcpy(&id, id128, sizeof(id));
  NCCL_TRY(r, r->CommInitRank(&c->comm, world, id, rank));
  guard.c = nullptr;
  *out = c;
  return 0;
}

void m4q_comm_destroy(m4q_comm* c) {
  if (!c) return;
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->comm) (void)rccl()->CommDestroy(c->comm);
  for (auto& e : c->slot) if (e) (void)hipEventDestroy(e);
  if (c->dep) (void)hipEventDestroy(c->dep);
  if (c->scratch) (void)hipFree(c->scratch);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

int m4q_comm_gather(m4q_comm* c, m4q_session* after, const void* send_dev, void* recv_dev, size_t bytes, int32_t dst, int32_t slot) {
  if (!c || !send_dev || bytes == 0 || dst < 0 || dst >= c->world || slot < 0 || slot >= 8 || (c->rank == dst && !recv_dev))
    return fail(M4Q_E_BADARG, "m4q_comm_gather: bad argument");
  Rccl* r = rccl();
  if (after) {
    HIP_TRY(hipEventRecord(c->dep, after->stream));
    HIP_TRY(hipStreamWaitEvent(c->stream, c->dep, 0));
  }
  NCCL_TRY(r, r->Gather(send_dev, recv_dev, bytes, ncclUint8, dst, c->comm, c->stream));
  HIP_TRY(hipEventRecord(c->slot[slot], c->stream));
  return 0;
}

int m4q_comm_wait(m4q_comm* c, int32_t slot) {
  if (!c || slot >= 8) return fail(M4Q_E_BADARG, "m4q_comm_wait: bad argument");
  if (slot < 0) HIP_TRY(hipStreamSynchronize(c->stream));
  else HIP_TRY(hipEventSynchronize(c->slot[slot]));
  return 0;
}

int m4q_comm_allreduce_f64(m4q_comm* c, double* inout_host, int32_t n, int32_t op) {
  if (!c || n < 0 || n > 64 || (n > 0 && !inout_host) || (op != 0 && op != 1)) return fail(M4Q_E_BADARG, "m4q_comm_allreduce_f64: bad argument");
  Rccl* r = rccl();
  double one = 0.0;
  const int cnt = n > 0 ? n : 1;                      // n = 0: a barrier (one dummy element)
  HIP_TRY(hipMemcpyAsync(c->scratch, n > 0 ? inout_host : &one, cnt * sizeof(double), hipMemcpyHostToDevice, c->stream));
  NCCL_TRY(r, r->AllReduce(c->scratch, c->scratch + 64, cnt, ncclDouble, op == 0 ? ncclSum : ncclMax, c->comm, c->stream));
  HIP_TRY(hipMemcpyAsync(n > 0 ? inout_host : &one, c->scratch + 64, cnt * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

int m4q_device_alloc(size_t bytes, int32_t device, void** out) {
  if (!out || bytes == 0) return fail(M4Q_E_BADARG, "m4q_device_alloc: bad argument");
  int rc = need_device();
  if (rc) return rc;
  if (device >= 0) HIP_TRY(hipSetDevice(device));
  void* p = nullptr;
  HIP_TRY(hipMalloc(&p, bytes));
  hipError_t e = hipMemset(p, 0, bytes);
  if (e != hipSuccess) { (void)hipFree(p); return fail(-(int)e, "hipMemset: %s", hipGetErrorString(e)); }
  *out = p;
  return 0;
}

int m4q_device_free(void* dev) {
  if (dev) HIP_TRY(hipFree(dev));
  return 0;
}

int m4q_device_read(void* host, const void* dev, size_t bytes) {
  if (!host || !dev) return fail(M4Q_E_BADARG, "m4q_device_read: bad argument");
  HIP_TRY(hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost));
  return 0;
}

int m4q_device_write(void* dev, const void* host, size_t bytes) {
  if (!host || !dev) return fail(M4Q_E_BADARG, "m4q_device_write: bad argument");
  HIP_TRY(hipMemcpy(dev, host, bytes, hipMemcpyHostToDevice));
  return 0;
}

}  // extern "C"
