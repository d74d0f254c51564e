// Timing builds only (POSERISK_CXXFLAGS=-DPR_TIMING_HOOKS; never in the shipped library): the host side of the kernels'
// clock stamps.  A launcher that stamps declares `static int calls` and, in front of its launch,
//     StampRecorder rec("POSERISK_X_STAMPS", words, 20, calls, stream);   args.stamps = rec.stamps();
// While the variable names a file, the fire_on-th such call of the process gets a zeroed device buffer of `words` 64-bit
// stamps (every other call gets nullptr and its kernel stamps nothing); when the launcher returns, the recorder waits for
// the stream, copies the buffer back and writes it to the file as it is, for the launcher's scripts/*_stamps.py to read.
#pragma once
#ifdef PR_TIMING_HOOKS
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

namespace pr {

class StampRecorder {
 public:
  StampRecorder(const char* env, size_t words, int fire_on, int& calls, hipStream_t stream) : words_(words), stream_(stream) {
    path_ = env ? getenv(env) : nullptr;   // env == nullptr: this call is not one that could be recorded, and is not counted
    if (!path_ || ++calls != fire_on) return;
    if (hipMalloc(&buf_, words * 8) != hipSuccess || hipMemsetAsync(buf_, 0, words * 8, stream) != hipSuccess) {
      (void)hipFree(buf_);
      buf_ = nullptr;
    }
  }
  StampRecorder(const StampRecorder&) = delete;
  StampRecorder& operator=(const StampRecorder&) = delete;
  unsigned long long* stamps() const { return buf_; }
  ~StampRecorder() {
    if (!buf_) return;
    std::vector<unsigned long long> host(words_);
    (void)hipStreamSynchronize(stream_);
    (void)hipMemcpy(host.data(), buf_, words_ * 8, hipMemcpyDeviceToHost);
    (void)hipFree(buf_);
    if (FILE* f = fopen(path_, "wb")) {
      fwrite(host.data(), 8, words_, f);
      fclose(f);
    }
  }

 private:
  const char* path_ = nullptr;
  unsigned long long* buf_ = nullptr;
  size_t words_;
  hipStream_t stream_;
};

}  // namespace pr
#endif  // PR_TIMING_HOOKS
