// The internal fence: device_alloc / device_free (fence.h) and the C entries that read the guards back.
#include "fence.h"

#include <mutex>
#include <string>
#include <vector>

namespace pr {
namespace {

struct FenceRecord {
  std::string name;
  char* raw = nullptr;      // what hipMalloc returned: guard | payload | guard
  size_t guard = 0, payload = 0;
  int device = 0;
};

std::mutex g_mu;
std::vector<FenceRecord> g_live;
std::atomic<int> g_n_live{0};              // device_free's fast path: nothing fenced, nothing to look up
std::vector<std::string> g_sticky;         // damage found when a fenced allocation was freed, until reported

std::string vformat(const char* fmt, va_list ap) {
  char buf[256];
  vsnprintf(buf, sizeof buf, fmt, ap);
  return buf;
}

// One guard of `r` read back and scanned; a damaged one is a line in `lines`.  front: offsets are relative to the payload's
// first byte (-1 = the byte before it); behind: to the byte after the payload's last (+0).
int scan_guard(const FenceRecord& r, bool front, std::vector<unsigned char>& host, std::vector<std::string>* lines) {
  host.resize(r.guard);
  const char* src = front ? r.raw : r.raw + r.guard + r.payload;
  PR_HIP(hipMemcpy(host.data(), src, r.guard, hipMemcpyDeviceToHost));
  const FenceScan s = fence_scan(host.data(), r.guard);
  if (!s.count) return PR_OK;
  char buf[512];
  if (front)
    snprintf(buf, sizeof buf, "%s (%zu bytes): guard IN FRONT touched: %zu bytes, first at -%zu, last at -%zu (bytes before the payload's first)",
             r.name.c_str(), r.payload, s.count, r.guard - s.first, r.guard - s.last);
  else
    snprintf(buf, sizeof buf, "%s (%zu bytes): guard BEHIND touched: %zu bytes, first at +%zu, last at +%zu (bytes past the payload's last)",
             r.name.c_str(), r.payload, s.count, s.first, s.last);
  lines->push_back(buf);
  return PR_OK;
}

int scan_record(const FenceRecord& r, std::vector<unsigned char>& host, std::vector<std::string>* lines) {
  DeviceGuard g(r.device);
  PR_HIP(hipDeviceSynchronize());
  PR_TRY(scan_guard(r, true, host, lines));
  return scan_guard(r, false, host, lines);
}

int write_report(const std::vector<std::string>& lines, char* report, size_t capacity) {
  size_t at = 0;
  if (report && capacity) report[0] = 0;
  for (const std::string& l : lines) {
    if (!report || at + l.size() + 2 > capacity) break;      // a report that does not fit is cut at a line; the count is whole
    memcpy(report + at, l.data(), l.size());
    at += l.size();
    report[at++] = '\n';
    report[at] = 0;
  }
  return (int)lines.size();
}

}  // namespace

int fence_mode_from_env() {
  const char* e = getenv("POSERISK_FENCE");
  const int v = e ? atoi(e) : 0;
  return v == 1 || v == 2 ? v : 0;
}

int device_alloc(void** out, size_t bytes, int mode, size_t frame_bytes, const char* name_fmt, ...) {
  if (!mode) {
    PR_HIP(hipMalloc(out, bytes));
    return PR_OK;
  }
  FenceRecord r;
  va_list ap;
  va_start(ap, name_fmt);
  r.name = vformat(name_fmt, ap);
  va_end(ap);
  r.guard = fence_guard_bytes(frame_bytes);
  r.payload = bytes;
  PR_HIP(hipGetDevice(&r.device));
  void* raw = nullptr;
  PR_HIP(hipMalloc(&raw, r.guard + bytes + r.guard));
  r.raw = (char*)raw;
  if (hipMemset(raw, kFenceFill, r.guard + bytes + r.guard) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
    (void)hipFree(raw);
    set_error("fence: filling %s failed", r.name.c_str());
    return PR_ERR_HIP;
  }
  *out = r.raw + r.guard;
  std::lock_guard<std::mutex> lock(g_mu);
  g_live.push_back(std::move(r));
  g_n_live.store((int)g_live.size(), std::memory_order_release);
  return PR_OK;
}

void device_free(void* p) {
  if (!p) return;
  if (g_n_live.load(std::memory_order_acquire)) {
    std::lock_guard<std::mutex> lock(g_mu);
    for (size_t i = 0; i < g_live.size(); ++i)
      if (g_live[i].raw + g_live[i].guard == (char*)p) {
        std::vector<unsigned char> host;
        (void)scan_record(g_live[i], host, &g_sticky);
        (void)hipFree(g_live[i].raw);
        g_live.erase(g_live.begin() + i);
        g_n_live.store((int)g_live.size(), std::memory_order_release);
        return;
      }
  }
  (void)hipFree(p);
}

void fence_rename(const void* p, const char* name_fmt, ...) {
  if (!p || !g_n_live.load(std::memory_order_acquire)) return;
  va_list ap;
  va_start(ap, name_fmt);
  const std::string name = vformat(name_fmt, ap);
  va_end(ap);
  std::lock_guard<std::mutex> lock(g_mu);
  for (FenceRecord& r : g_live)
    if (r.raw + r.guard == (const char*)p) r.name = name;
}

}  // namespace pr

extern "C" {

int pr_fence_check(char* report, size_t capacity) {
  using namespace pr;
  if (report && capacity) report[0] = 0;
  PR_TRY(refuse_under_declared_capture("pr_fence_check"));
  std::lock_guard<std::mutex> lock(g_mu);
  std::vector<std::string> lines;
  lines.swap(g_sticky);
  std::vector<unsigned char> host;
  for (const FenceRecord& r : g_live)
    if (scan_record(r, host, &lines) != PR_OK) lines.push_back(r.name + ": the guards could not be read back: " + pr_last_error());
  return write_report(lines, report, capacity);
}

int pr_fence_list(char* report, size_t capacity) {
  using namespace pr;
  std::lock_guard<std::mutex> lock(g_mu);
  std::vector<std::string> lines;
  for (const FenceRecord& r : g_live) {
    char buf[400];
    snprintf(buf, sizeof buf, "%s\t%zu\t%zu", r.name.c_str(), r.payload, r.guard);
    lines.push_back(buf);
  }
  return write_report(lines, report, capacity);
}

int pr_fence_payload_fill(const char* name, size_t* leading, size_t* trailing) {
  using namespace pr;
  PR_REQUIRE(name && leading && trailing, "pr_fence_payload_fill: null argument");
  PR_TRY(refuse_under_declared_capture("pr_fence_payload_fill"));
  std::lock_guard<std::mutex> lock(g_mu);
  for (const FenceRecord& r : g_live)
    if (r.name == name) {
      PR_REQUIRE(r.payload <= ((size_t)256 << 20), "pr_fence_payload_fill: %s holds %zu bytes, more than this entry reads back", name, r.payload);
      DeviceGuard g(r.device);
      PR_HIP(hipDeviceSynchronize());
      std::vector<unsigned char> host(r.payload);
      PR_HIP(hipMemcpy(host.data(), r.raw + r.guard, r.payload, hipMemcpyDeviceToHost));
      size_t a = 0, b = 0;
      while (a < r.payload && host[a] == kFenceFill) ++a;
      while (b < r.payload && host[r.payload - 1 - b] == kFenceFill) ++b;
      *leading = a;
      *trailing = b;
      return PR_OK;
    }
  set_error("pr_fence_payload_fill: no live fenced allocation is named %s", name);
  return PR_ERR_INVALID;
}

int pr_fence_selftest(void) {
  using namespace pr;
  PR_TRY(refuse_under_declared_capture("pr_fence_selftest"));
  const size_t bytes = 4096;
  void* p = nullptr;
  PR_TRY(device_alloc(&p, bytes, 1, 0, "fence selftest"));      // fenced whatever the switch says
  int bad = 0;
  std::vector<std::string> lines;
  std::vector<unsigned char> host;
  {
    std::lock_guard<std::mutex> lock(g_mu);
    const FenceRecord r = g_live.back();
    if (r.raw + r.guard != (char*)p || r.guard != kFenceMinGuard) ++bad;
    if (scan_record(r, host, &lines) != PR_OK || !lines.empty()) ++bad;      // fresh guards are intact
    // one byte directly in front of the payload, one directly behind it: both inside this allocation
    if (hipMemset((char*)p - 1, 0, 1) != hipSuccess || hipMemset((char*)p + bytes, 0, 1) != hipSuccess) ++bad;
    lines.clear();
    if (scan_record(r, host, &lines) != PR_OK || lines.size() != 2) ++bad;
    else {
      if (lines[0].find("fence selftest (4096 bytes): guard IN FRONT touched: 1 bytes, first at -1, last at -1 ") != 0) ++bad;
      if (lines[1].find("fence selftest (4096 bytes): guard BEHIND touched: 1 bytes, first at +0, last at +0 ") != 0) ++bad;
    }
  }
  // the free finds the same two regions and keeps them: exactly those, and they are cleared here
  device_free(p);
  std::lock_guard<std::mutex> lock(g_mu);
  size_t mine = 0;
  for (size_t i = 0; i < g_sticky.size();)
    if (g_sticky[i].find("fence selftest ") == 0) {
      g_sticky.erase(g_sticky.begin() + i);
      ++mine;
    } else {
      ++i;
    }
  if (mine != 2) ++bad;
  return bad;
}

}  // extern "C"
