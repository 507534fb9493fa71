// Device-side entry points of the per-party protocol kernels (rss_party.hip, rss_jobs.hip),
// called by the host / device dispatchers mx_* of rss_party_cpu.cpp and rss_jobs_cpu.cpp.
// Internal: the definitions and the callers both include this header, so a signature cannot
// drift between them.
#pragma once
#include <stdint.h>

extern "C" {
int mxh_trunc_party_r0(int words, int64_t n, int m, int ncomp, const int* roles,
                       const void* s0, const void* s1, void* msg, void* msg_rm, void* out0,
                       void* out1, const uint32_t* const* slots, const uint64_t* nn,
                       void* stream);
int mxh_trunc_party_r1(int words, int64_t n, int m, int ncomp, const int* roles,
                       const void* msg, const void* rmk, const void* rrt, const void* rrm,
                       void* w, void* out0, void* out1, const uint32_t* const* slots,
                       const uint64_t* nn, void* stream);
int mxh_ring_extend_party_r0(int64_t n, int ncomp, const int* roles, const void* s0,
                             const void* s1, void* msg, void* msg_R, void* msg_M, void* out0,
                             void* out1, const uint32_t* const* slots, const uint64_t* nn,
                             void* stream);
int mxh_ring_extend_party_r1(int64_t n, int ncomp, const int* roles, const void* msg,
                             const void* rmk, const void* rR, const void* rM, void* w,
                             void* out0, void* out1, const uint32_t* const* slots,
                             const uint64_t* nn, void* stream);
int mxh_share_party(int kind, int words, int64_t n, int ncomp, const int* rel, const void* x,
                    void* out0, void* out1, const uint32_t* const* slots, uint64_t n1,
                    uint64_t na, void* stream);
int mxh_dot_tail_r0(int words, int64_t n, int m, int ncomp, const int* roles,
                    const void* const* cross, void* const* msg, void* const* msg_rt,
                    void* const* msg_rm, void* const* out0, void* const* out1,
                    const uint32_t* const* slots, const uint64_t* nn, void* stream);
int mxh_dot_tail_r1(int words, int64_t n, int m, int ncomp, const int* roles,
                    const void* const* msg, const void* const* rmk, const void* const* rz,
                    const void* const* rrt, const void* const* rrm, void* const* w,
                    void* const* out0, void* const* out1, const uint32_t* const* slots,
                    const uint64_t* nn, void* stream);
int mxh_dot_tail_r2(int words, int64_t n, int ncomp, const int* roles, const void* const* a,
                    const void* const* b, void* const* out, void* stream);

int mxh_jobs_r0(int words, int njobs, const void* const* ptrs, const int64_t* dims, int64_t L,
                int m, int role, int main, int dealer, void* msg, void* msg_rt, void* msg_rm,
                const uint32_t* const* slots, const uint64_t* nn, void* stream);
int mxh_jobs_r0p(int words, int njobs, const void* const* ptrs, const int64_t* dims, int64_t L,
                 int m, int role, int main, int dealer, void* msg, void* msg_rt, void* msg_rm,
                 const uint32_t* const* slots, const uint64_t* nn, int npend,
                 const void* const* pend, const int64_t* pend_len, void* stream);
int mxh_jobs_r1(int words, int njobs, const void* const* ptrs, const int64_t* dims, int64_t L,
                int m, int role, const void* msg, const void* rmk, const void* rz,
                const void* rrt, const void* rrm, void* w, const uint32_t* const* slots,
                const uint64_t* nn, void* stream);
int mxh_jobs_r2(int words, int njobs, const void* const* ptrs, const int64_t* dims, int64_t L,
                int role, const void* a, const void* b, void* stream);
}
