// pre3_icp.h -- the constants, the state block and the loop-control rule of the dense ICP between two point clouds (pre3_icp.hip).
//   TestScripts/icp_with_init.m:37-39,46-48,63-75,90-100  (maxIter, c1 / c2, n, e1 / e2, noChangeCount, error)
// __host__ __device__, so that a host program can step the rule (tests/icp_host_main.cpp, tests/test_icp_loop_host.py).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PRE3_ICP_HD __host__ __device__ inline
#else
#define PRE3_ICP_HD inline
#endif

namespace pre3 {

constexpr int ICP_PTS = 4;                          // source points a lane of k_icp_nn keeps in registers
constexpr int ICP_NN_THREADS = 256;
constexpr int ICP_SRC_TILE = ICP_NN_THREADS * ICP_PTS;     // source points per workgroup
constexpr int ICP_CHUNK = 256;                      // model points a workgroup stages in LDS (3 x 2 KB): 25 x 99 workgroups at 144 x 176, DESIGN.md section 31
constexpr int ICP_MAX_ITER = 30;                    // icp_with_init.m:37
constexpr int ICP_ITER_CAP = 2 * (ICP_MAX_ITER + 1);      // each phase ends at n > maxIter: 31 + 31 iterations at most
constexpr int ICP_NOCHANGE = 10;                    // :74

// status of a run
constexpr int ICP_NOT_RUN = 0, ICP_OK = 1, ICP_FEW = 2, ICP_NONFINITE = 3;

// the state block one thread advances once per iteration: 96 bytes
struct IcpCtl {
    int32_t phase;          // 1: :47-68, 2: :74-99
    int32_t n;              // the phase's own iteration counter
    int32_t c1, c2;         // :38-39, :48, :63
    int32_t no_change;      // :73, :96-98
    int32_t done, status;
    int32_t it1, it2;       // iterations run in either phase (one that found p < 3 included)
    int32_t total;          // it1 + it2: the next row of the log
    int32_t p;              // the last iteration's correspondence count
    int32_t apply_seq;      // total after the last iteration that produced a transform: its apply launch compares it with its own number
    double e1, e2;          // :70-71, :75, :90
    double res;
    double last_e;          // sum(D) / (p res) of the last iteration, either phase (the log's third column)
    int32_t n1, n2;         // points of the model and of the source
    int32_t pad[2];
};

PRE3_ICP_HD void icp_ctl_start(IcpCtl *c, int n1, int n2, double res)
{
    c->phase = 1; c->n = 0; c->c1 = 0; c->c2 = 1; c->no_change = 0; c->done = 0; c->status = ICP_NOT_RUN;
    c->it1 = c->it2 = c->total = 0; c->p = 0; c->apply_seq = 0;
    c->e1 = 1000001.0; c->e2 = 1000000.0; c->res = res; c->last_e = 0.0;
    c->n1 = n1; c->n2 = n2; c->pad[0] = c->pad[1] = 0;
}

// One iteration has found p correspondences whose distances sum to sum_d.  Returns 1 when the iteration's transform is to be applied (p >= 3).
// length(corr) of a p x 3 array is max(p, 3) and the reference fails at p = 0: here p < 3 ends the run with ICP_FEW and no transform.
PRE3_ICP_HD int icp_advance(IcpCtl *c, int p, double sum_d)
{
#pragma clang fp contract(off)
    if (c->done) return 0;
    c->total += 1;
    if (c->phase == 1) c->it1 += 1; else c->it2 += 1;
    c->p = p;
    if (p < 3) { c->done = 1; c->status = ICP_FEW; c->last_e = 0.0; return 0; }
    const double e = sum_d / ((double)p * c->res);          // :90
    c->last_e = e;
    if (c->phase == 1) {
        c->c1 = c->c2;                                      // :48
        c->c2 = p;                                          // :63
        c->n += 1;
        if (c->n > ICP_MAX_ITER || c->c2 == c->c1) { c->phase = 2; c->n = 0; c->no_change = 0; c->e1 = 1000001.0; c->e2 = 1000000.0; }      // :65-67, :47, :70-73
    } else {
        c->e1 = c->e2;                                      // :75
        c->e2 = e;
        c->n += 1;
        if (c->n > ICP_MAX_ITER) { c->done = 1; c->status = ICP_OK; }                       // :93-95, ahead of the no-change test
        else {
            const double de = c->e2 - c->e1;
            if ((de < 0 ? -de : de) < c->res / 10000) c->no_change += 1;                    // :96-98
            if (c->no_change >= ICP_NOCHANGE) { c->done = 1; c->status = ICP_OK; }          // :74
        }
    }
    c->apply_seq = c->total;
    return 1;
}

PRE3_ICP_HD double icp_error(const IcpCtl *c) { return c->e1 < c->e2 ? c->e1 : c->e2; }      // :100

}  // namespace pre3

#if defined(__HIPCC__)
#include "pre3_internal.h"
#include <mutex>
namespace pre3 {
struct VoOut; struct VoCov;
// what a call hands out (each may be null): corr [p][3] = (model, source, D), 1-based; corr_pix [p][2] pixel indices (frames only); data2 3 x n2; log [62][3]
// cov [49], cov_status: the closed-form covariance of u behind the run (IcpJob::with_cov; pre3_icpcov.h)
struct IcpOutputs { pre3_icp_result *res; double *corr; int32_t *corr_pix; double *data2; double *log; double *cov = nullptr; int32_t *cov_status = nullptr; };
// one run in flight: its device block, the lock on the library's pinned result block, and what the host needs to decode it after the wait
struct IcpJob {
    Scratch dev;
    std::unique_lock<std::mutex> pin_lock;
    char *pin = nullptr;
    hipStream_t st = nullptr;
    bool queued = false, waited = false, frames = false;
    int cap1 = 0, cap2 = 0;
    size_t o_corr_m = 0, o_corr_s = 0, o_corr_d = 0, o_src = 0, o_mpix = 0, o_spix = 0, pin_bytes = 0;
    // set by the caller before the run is queued (frames forms): k_icp_cov_part / k_icp_cov_fin behind k_icp_final, their VoCov block and partials at the
    // end of the device block, the VoCov block transferred behind the front of the pinned one
    bool with_cov = false;
    size_t o_cov = 0, o_part = 0, o_pin_cov = 0;
    const double *cov_x = nullptr, *cov_y = nullptr, *cov_z = nullptr;      // the source frame's filtered planes, read through spix
    int cov_npix = 0;
    // set by the caller before the run is queued: the device block comes from an owner that outlives the run (block(owner, bytes, &d)) instead of `dev`,
    // and the head is built by a launch instead of uploaded from the pinned block -- nothing of a run that no host waits for hangs on this object or on
    // the library's pinned block.  pin_back: the results are still transferred (the caller waits and collects); otherwise the pinned block is not touched
    int (*block)(void *owner, size_t bytes, char **out) = nullptr;
    void *owner = nullptr;
    bool pin_back = true;
    char *d = nullptr;              // the device block in use, either way
    IcpJob() = default;
    IcpJob(const IcpJob &) = delete;
    ~IcpJob() { if (queued && !waited && pin_back) (void)hipStreamSynchronize(st); }      // an error path: nothing queued may outlive the blocks it holds
    size_t o_taken = 0, o_pin_taken = 0;        // with `block`: two int32 a launch behind the run reports in (pre3_predict_icp_pair_seeded's taken_out)
};
// where a run's launches leave what a launch behind them reads (IcpJob::with_cov for cov, IcpJob::block for taken)
struct IcpDevView { const IcpCtl *ctl; const double *u, *error; const VoCov *cov; int32_t *taken; };
void icp_job_dev_view(const IcpJob *job, IcpDevView *v);
// the model is every pixel of v1's filtered planes as [-x; -y; z], the source v2's pixels at rows and columns 0, stride, ...; Rinit / Tinit from the host,
// or (vo_dev != nullptr) from a VO pair's result block on the device, in which case a pair that did not end in sta == 1 leaves the run at ICP_NOT_RUN.
// Everything is queued on st, the transfer of the results included; the caller waits for st, then calls icp_job_collect.
int icp_job_queue_frames(IcpJob *job, const SrFrameView &v1, const SrFrameView &v2, int stride, double res, const double *Rinit, const double *Tinit,
                         const VoOut *vo_dev, const IcpOutputs &want, hipStream_t st);
int icp_job_collect(IcpJob *job, const char *who, const IcpOutputs &o);
int icp_check_args(const char *who, int stride, double res);
}  // namespace pre3
#endif
