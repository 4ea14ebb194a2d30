// C-ABI implementation of libccmm (include/ccmm.h), host code only.  This unit: the thread's error string, the
// options and environment tables, contexts, the MFMA phase-lock registry and the MFMA self-tests.  The chain set is
// declared in ccmm_chains.h and implemented block by block in ccmm_chains.hip / ccmm_chains_sweep.hip /
// ccmm_chains_elb.hip / ccmm_chains_fcst.hip, each ending in the entry points of its block; the block-level
// drop-ins are in ccmm_dropins.hip, the pure host arithmetic in ccmm_host_math.hip.  The kernels are defined in
// their own translation units (ccmm_kernels / ccmm_gram_chol / ccmm_cta_solve / ccmm_elb / ccmm_ps / ccmm_fcst /
// ccmm_lag / ccmm_svpart / ccmm_big / ccmm_bign / ccmm_post / ccmm_girf), each with the host launchers of its
// templated kernels; their headers hold the LDS sizes and the launch decisions the host units read.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>

#include "ccmm_host.h"
#include "ccmm_sweep.h"

using namespace ccmm;

namespace ccmm {
thread_local std::string g_err;  // the one error string of a thread: every unit goes through the two accessors
void set_last_error(const std::string& msg) { g_err = msg; }
const std::string& last_error() { return g_err; }
}  // namespace ccmm

// the MFMA phase locks of the process, by (device, id)
PhaseLock& phase_lock(int device, int id) {
  static std::mutex gm;
  static std::map<std::pair<int, int>, std::unique_ptr<PhaseLock>> locks;
  std::lock_guard<std::mutex> g(gm);
  auto& p = locks[{device, id}];
  if (!p) p.reset(new PhaseLock);
  return *p;
}

// ---------------------------------------------------------------- environment switches
namespace {
// timing-only ablations (results invalid), with the selector bits a default build still honours
struct AblationVar {
  const char* name;
  int keep_mask;
};
const AblationVar kAblationVars[] = {
    {"CCMM_CHOL_SKIP", 0},  {"CCMM_SOLVE_SKIP", 0}, {"CCMM_SV_SKIP", 0},  {"CCMM_GC_MODE", 0},
    {"CCMM_LAG_MODE", 0},   {"CCMM_BIG_MASK", 0},   {"CCMM_ELB_MODE", 0}, {"CCMM_SV_MODE", 0},
    {"CCMM_FCST_MODE", 0},  {"CCMM_POISON", 0},
};
// an ablation variable is "ignored" when it is set and a bit outside its keep_mask is non-zero
bool ablation_ignored(const AblationVar& v) {
#ifdef CCMM_ABLATION
  (void)v;
  return false;
#else
  const char* e = std::getenv(v.name);
  return e && (std::atoi(e) & ~v.keep_mask) != 0;
#endif
}
// an option's variable is "ignored" by a default build whenever it is set
bool option_env_ignored(int i) {
#ifdef CCMM_ABLATION
  (void)i;
  return false;
#else
  return std::getenv(kOptDesc[i].env) != nullptr;
#endif
}
// switches of kernels that no longer exist (round 5 and before): read by no build
const char* const kRetiredVars[] = {"CCMM_OLD_SOLVE", "CCMM_OLD_CHOL", "CCMM_GC18", "CCMM_NO_LAG",
                                    "CCMM_NO_QR_FALLBACK", "CCMM_SOLVE_WAVES"};
}  // namespace

std::string ignored_list() {
  std::string out;
  for (const auto& v : kAblationVars)
    if (ablation_ignored(v)) out += (out.empty() ? "" : ",") + std::string(v.name);
  for (const char* r : kRetiredVars)
    if (std::getenv(r)) out += (out.empty() ? "" : ",") + std::string(r);
  for (int i = 0; i < kOptCount; ++i)
    if (option_env_ignored(i)) out += (out.empty() ? "" : ",") + std::string(kOptDesc[i].env);
  return out;
}

const ccmm::OptDesc ccmm::kOptDesc[ccmm::kOptCount] = {
    {"solve_split", "CCMM_SOLVE_SPLIT", -1, -1, 1},
    {"solve_async", "CCMM_SOLVE_ASYNC", 1, 0, 1},
    {"sv_nwg", "CCMM_SV_NWG", 0, 0, 4},
    {"elb_waves", "CCMM_ELB_WAVES", 8, 1, 8},
    {"elb_oct", "CCMM_ELB_OCT", 1, 0, 2},
    {"elb_async", "CCMM_ELB_ASYNC", 1, 0, 1},
    {"elb_parts", "CCMM_ELB_PARTS", 0, 0, 4},
    {"elb_spec", "CCMM_ELB_SPEC", 0, 0, 1},
    {"fcst_reg", "CCMM_FCST_REG", 1, 0, 1},
    {"fcst_overlap", "CCMM_FCST_OVERLAP", 1, 0, 1},
    {"phi_overlap", "CCMM_PHI_OVERLAP", 1, 0, 1},
    {"qr_fallback", "CCMM_QR_FALLBACK", 1, 0, 1},
    {"big_lagx", "CCMM_BIG_LAGX", 1, 0, 1},
    {"phi_stage", "CCMM_PHI_STAGE", 3, 0, 3},
    {"lag", "CCMM_LAG", 1, 0, 1},
    {"large_path", "CCMM_FORCE_BIG", 0, 0, 1},
    {"astep_serial", "CCMM_ASTEP_V1", 0, 0, 1},
    {"ps_chol_lds", "CCMM_PS_CHOL_V1", 0, 0, 1},
    {"sv_mfma", "CCMM_SV_MFMA", 1, 0, 1},
    {"force_qr", "CCMM_FORCE_QR", 0, 0, 1},
    {"girf_generic", "CCMM_GIRF_GENERIC", 0, 0, 1},
};

ccmm::Options::Options() {
  for (int i = 0; i < kOptCount; ++i) {
    v[i] = kOptDesc[i].dflt;
#ifdef CCMM_ABLATION
    if (const char* e = std::getenv(kOptDesc[i].env)) v[i] = std::max(kOptDesc[i].lo, std::min(kOptDesc[i].hi, std::atoi(e)));
#endif
  }
}

int ccmm::option_id(const char* name) {
  if (!name) return -1;
  for (int i = 0; i < kOptCount; ++i)
    if (std::strcmp(name, kOptDesc[i].name) == 0) return i;
  return -1;
}

int ccmm::env_ablation(const char* name, int off, int keep_mask) {
  const char* e = std::getenv(name);
  if (!e) return off;
#ifdef CCMM_ABLATION
  (void)keep_mask;
  return std::atoi(e);
#else
  return (off & ~keep_mask) | (std::atoi(e) & keep_mask);
#endif
}

int set_opt(Options& o, const char* name, int value) {
  const int i = option_id(name);
  if (i < 0) {
    set_last_error(std::string("unknown option '") + (name ? name : "(null)") + "'");
    return CCMM_ERR_ARG;
  }
  if (value < kOptDesc[i].lo || value > kOptDesc[i].hi) {
    set_last_error(std::string("option '") + name + "' out of range [" + std::to_string(kOptDesc[i].lo) + ", " +
                   std::to_string(kOptDesc[i].hi) + "]");
    return CCMM_ERR_ARG;
  }
  o.v[i] = value;
  return CCMM_OK;
}

int get_opt(const Options& o, const char* name, int* value) {
  const int i = option_id(name);
  if (i < 0 || !value) {
    set_last_error(std::string("unknown option '") + (name ? name : "(null)") + "'");
    return CCMM_ERR_ARG;
  }
  *value = o.v[i];
  return CCMM_OK;
}

extern "C" {

int ccmm_abi_version(void) { return CCMM_ABI_VERSION; }
const char* ccmm_last_error(void) { return last_error().c_str(); }

int ccmm_ablation_build(void) {
#ifdef CCMM_ABLATION
  return 1;
#else
  return 0;
#endif
}

int ccmm_env_ignored(char* buf, int len) {
  const std::string l = ignored_list();
  if (buf && len > 0) {
    const size_t n = std::min((size_t)len - 1, l.size());
    std::memcpy(buf, l.data(), n);
    buf[n] = 0;
  }
  int count = l.empty() ? 0 : 1;
  for (char ch : l) count += ch == ',' ? 1 : 0;
  return count;
}

int ccmm_option_count(void) { return kOptCount; }

const char* ccmm_option_name(int i) { return (i >= 0 && i < kOptCount) ? kOptDesc[i].name : nullptr; }

int ccmm_option_default(const char* name, int* value) {
  const Options o;  // what a new context starts from (a default build: the built-in values)
  return get_opt(o, name, value);
}

int ccmm_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

ccmm_ctx* ccmm_create(int device) {
  ccmm_ctx* ctx = nullptr;
  int rc = guarded([&] {
    int n = 0;
    HIPCHECK(hipGetDeviceCount(&n));
    require(device >= 0 && device < n, "device index out of range");
    HIPCHECK(hipSetDevice(device));
    ctx = new ccmm_ctx;
    ctx->device = device;
    // a BLOCKING stream: host uploads use hipMemcpy on the null stream, and a pageable
    // host-to-device copy may return before its DMA has landed; only a stream that
    // synchronises with the null stream orders the kernels after it
    HIPCHECK(hipStreamCreateWithFlags(&ctx->stream, hipStreamDefault));
    return 0;
  });
  if (rc != 0) {
    delete ctx;
    return nullptr;
  }
  return ctx;
}

void ccmm_destroy(ccmm_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

int ccmm_set_option(ccmm_ctx* ctx, const char* name, int value) {
  if (!ctx) {
    set_last_error("null context");
    return CCMM_ERR_ARG;
  }
  return set_opt(ctx->opt, name, value);
}

int ccmm_get_option(ccmm_ctx* ctx, const char* name, int* value) {
  if (!ctx) {
    set_last_error("null context");
    return CCMM_ERR_ARG;
  }
  return get_opt(ctx->opt, name, value);
}

int ccmm_synchronize(ccmm_ctx* ctx) {
  return guarded([&] {
    require(ctx != nullptr, "null context");
    HIPCHECK(hipSetDevice(ctx->device));
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    return 0;
  });
}

int ccmm_selftest_mfma_f64(ccmm_ctx* ctx, const double* A16x4, const double* B4x16, double* D16x16) {
  return guarded([&] {
    require(ctx && A16x4 && B4x16 && D16x16, "null argument");
    HIPCHECK(hipSetDevice(ctx->device));
    DBuf<double> a, b, dd;
    a.alloc(64);
    b.alloc(64);
    dd.alloc(256);
    HIPCHECK(hipMemcpy(a.p, A16x4, 64 * sizeof(double), hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(b.p, B4x16, 64 * sizeof(double), hipMemcpyHostToDevice));
    HIPCHECK(launch_mfma_selftest(ctx->stream, a.p, b.p, dd.p));
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    HIPCHECK(hipMemcpy(D16x16, dd.p, 256 * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
  });
}

int ccmm_selftest_mfma_f64_acc(ccmm_ctx* ctx, int nprobe, const double* A16x4, const double* B4x16,
                               const double* C16x16, double* D16x16) {
  return guarded([&] {
    require(ctx && A16x4 && B4x16 && C16x16 && D16x16 && nprobe > 0 && nprobe <= (1 << 20), "bad argument");
    HIPCHECK(hipSetDevice(ctx->device));
    DBuf<double> a, b, cc, dd;
    a.alloc((size_t)64 * nprobe);
    b.alloc((size_t)64 * nprobe);
    cc.alloc((size_t)256 * nprobe);
    dd.alloc((size_t)256 * nprobe);
    HIPCHECK(hipMemcpy(a.p, A16x4, (size_t)64 * nprobe * sizeof(double), hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(b.p, B4x16, (size_t)64 * nprobe * sizeof(double), hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(cc.p, C16x16, (size_t)256 * nprobe * sizeof(double), hipMemcpyHostToDevice));
    HIPCHECK(launch_mfma_selftest_acc(ctx->stream, a.p, b.p, cc.p, dd.p, nprobe));
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    HIPCHECK(hipMemcpy(D16x16, dd.p, (size_t)256 * nprobe * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
  });
}

}  // extern "C"
