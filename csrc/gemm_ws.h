// Per-stream scratch of the GEMM paths: gemm_mfma.hip and gemm_crt.hip each keep one
// StreamScratch, so the two never share a buffer.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>

// gemm_mfma.hip: capture-safe allocation, and the counters behind mx_workspace_*
bool mx_ws_malloc(void** p, int64_t bytes);
void mx_ws_note(int dev, int64_t want, bool ok);
void mx_ws_shared_note(void);

// Grow-only scratch per (device, stream): GEMMs issued on different streams (dataflow lanes,
// pipelined steps, the in-process parties' graphs replayed concurrently) may run at the same
// time and must not share residue buffers.  kPerDev exceeds the streams a process can hold
// (PyTorch's pools: 32 per priority, plus the null stream); past it streams would share the
// last slot (ordered only by the caller) -- counted, mx_workspace_shared_count.  Replaced
// buffers are retired, never freed (a captured graph may hold them).
class StreamScratch {
  struct Slot {
    void* ptr = nullptr;
    int64_t bytes = 0;
    hipStream_t stream = nullptr;
    bool used = false;
  };
  static constexpr int kPerDev = 128;
  std::mutex mu_;
  Slot slots_[16][kPerDev];

 public:
  void* get(int64_t bytes, hipStream_t st) {
    int dev = 0;
    hipGetDevice(&dev);
    if (dev < 0 || dev >= 16) return nullptr;
    std::lock_guard<std::mutex> lk(mu_);
    Slot* slot = nullptr;
    for (int i = 0; i < kPerDev && !slot; ++i)
      if (slots_[dev][i].used && slots_[dev][i].stream == st) slot = &slots_[dev][i];
    for (int i = 0; i < kPerDev && !slot; ++i)
      if (!slots_[dev][i].used) {
        slot = &slots_[dev][i];
        slot->used = true;
        slot->stream = st;
      }
    if (!slot) {
      slot = &slots_[dev][kPerDev - 1];
      mx_ws_shared_note();
    }
    Slot& w = *slot;
    if (w.bytes < bytes) {
      int64_t want = 1 << 20;
      while (want < bytes) want <<= 1;
      void* p = nullptr;
      const bool ok = mx_ws_malloc(&p, want);
      mx_ws_note(dev, want, ok);
      if (!ok) return nullptr;
      w.ptr = p;  // the previous buffer (if any) stays allocated
      w.bytes = want;
    }
    return w.ptr;
  }
};
