// What every host unit of libccmm shares (ccmm_abi / ccmm_chains* / ccmm_dropins / ccmm_host_math): error
// handling, device buffers, the context, the kernel ids of the profile and the MFMA phase lock.  Everything
// with static storage is declared here and defined once (ccmm_abi.hip unless noted).
#pragma once
#include <cstdlib>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "ccmm_err.h"
#include "ccmm_fcst.h"  // GLNodes (and ccmm_internal.h)

struct HipError : std::runtime_error {
  using std::runtime_error::runtime_error;
};
struct ArgError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

#define HIPCHECK(x)                                                                        \
  do {                                                                                     \
    hipError_t e_ = (x);                                                                   \
    if (e_ != hipSuccess)                                                                  \
      throw HipError(std::string(#x) + ": " + hipGetErrorString(e_) + " (" __FILE__ ":" + \
                     std::to_string(__LINE__) + ")");                                      \
  } while (0)

template <class F>
int guarded(F&& f) {
  try {
    return f();
  } catch (const ArgError& e) {
    ccmm::set_last_error(e.what());
    return CCMM_ERR_ARG;
  } catch (const HipError& e) {
    ccmm::set_last_error(e.what());
    return CCMM_ERR_HIP;
  } catch (const std::exception& e) {
    ccmm::set_last_error(e.what());
    return CCMM_ERR_HIP;
  }
}

inline void require(bool ok, const char* msg) {
  if (!ok) throw ArgError(msg);
}

template <class T>
struct DBuf {
  T* p = nullptr;
  size_t n = 0;
  void alloc(size_t count) {
    if (count <= n && p) return;
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
    if (count == 0) return;
    HIPCHECK(hipMalloc(&p, count * sizeof(T)));
    n = count;
    // debug: CCMM_POISON=1 fills new allocations with 0xFF bytes (NaN doubles) to expose
    // reads of never-written device memory
#ifdef CCMM_ABLATION
    static const bool poison = std::getenv("CCMM_POISON") != nullptr;
    if (poison) HIPCHECK(hipMemset(p, 0xFF, count * sizeof(T)));
#endif
  }
  ~DBuf() {
    if (p) (void)hipFree(p);
  }
};

struct ccmm_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  ccmm::Options opt;  // inherited by the chain sets created on it and used by the block-level drop-ins
};

enum KernelId {
  KID_RESID,
  KID_WEIGHTS,
  KID_SOLVE,
  KID_ASTEP,
  KID_SVMIX,
  KID_SVSAMPLE,
  KID_PHIGEN,
  KID_PHI,
  KID_STORE,
  KID_GRAMCHOL,
  KID_ELBPREP,
  KID_ELBCOND,
  KID_ELBGIBBS,
  KID_ELBREBUILD,
  KID_GRAMLAG,
  KID_SOLVELAG,
  KID_FCST,
  KID_GRAMBIG,
  KID_CHOLBIG,
  KID_SOLVEBIG,
  KID_ASTEPBIG,
  KID_SVBIG,
  KID_PHIBIG,
  KID_PSCHOL,
  KID_PSPROP,
  KID_EIG,
  KID_STATSEL,
  KID_DIAG,
  KID_GIRFPREP,
  KID_GIRF,
  KID_GIRFRB,
  KID_GIRFCOLLECT,
  KID_CONDMEAN,
  KID_VMA,
  KID_SUMFFR,
  KID_POSTGATHER,
  KID_POSTSTATS,
  KID_COUNT
};
extern const char* const kKernelNames[KID_COUNT];  // ccmm_chains.hip

// options and environment switches (ccmm_abi.hip): set_opt / get_opt return CCMM_OK or set the error string;
// ignored_list names the CCMM_* variables that are set and that this build does not read
int set_opt(ccmm::Options& o, const char* name, int value);
int get_opt(const ccmm::Options& o, const char* name, int* value);
std::string ignored_list();

// MFMA phase lock: chain sets given the same id (ccmm_chains_set_mfma_lock) on one device
// serialise their CTA Gram + Cholesky phase through a cross-stream event, so the groups fall
// out of step and one group's per-chain sequential blocks (CTA solve, SV, ELB Gibbs) run
// beside another group's MFMA phase instead of all groups contending for the CUs at once.
struct PhaseLock {
  std::mutex m;
  hipEvent_t last = nullptr;  // event recorded after the latest enqueued locked phase
};
PhaseLock& phase_lock(int device, int id);  // the one registry of the process

// One locked phase of a chain set (id > 0; else a no-op): takes the lock and orders the stream after the
// latest locked phase; release() records the set's event after this one and publishes it.
struct PhaseScope {
  std::unique_lock<std::mutex> lk;
  PhaseLock* L = nullptr;
  hipStream_t st;
  hipEvent_t& ev;
  PhaseScope(int device, int id, hipStream_t stream, hipEvent_t& event) : st(stream), ev(event) {
    if (id <= 0) return;
    L = &phase_lock(device, id);
    lk = std::unique_lock<std::mutex>(L->m);
    if (L->last) HIPCHECK(hipStreamWaitEvent(st, L->last, 0));
    if (!ev) HIPCHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  }
  void release() {
    if (!L) return;
    HIPCHECK(hipEventRecord(ev, st));
    L->last = ev;
    lk.unlock();
  }
};

// Two events of a fork / join between two streams, created on first use
struct EventPair {
  hipEvent_t fork = nullptr, join = nullptr;
  void ensure() {
    if (fork) return;
    HIPCHECK(hipEventCreateWithFlags(&fork, hipEventDisableTiming));
    HIPCHECK(hipEventCreateWithFlags(&join, hipEventDisableTiming));
  }
  ~EventPair() {
    if (fork) (void)hipEventDestroy(fork);
    if (join) (void)hipEventDestroy(join);
  }
};

// ---------------------------------------------------------------- host arithmetic (ccmm_host_math.hip)
// small dense host helpers (N <= 128): lower Cholesky and SPD inverse, column-major
void host_chol(std::vector<double>& A, int n);
std::vector<double> host_spd_inverse(const std::vector<double>& A, int n);
// A = P(2:Ny+1, :) \ I for P of K rows (column-major): forward substitution when `lower`, else Gauss-Jordan
// with partial pivoting; false: singular
bool host_struct_inverse(const double* P, int K, int Ny, bool lower, double* A);
ccmm::GLNodes make_gl_nodes();
const ccmm::GLNodes& gl_nodes();  // make_gl_nodes(), computed once
double host_erfcinv(double y);
