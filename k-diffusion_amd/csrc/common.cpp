// Error reporting + per-launch event timing shared by all entry points of libkdiff_hip.so.
#include "kd_common.h"
#include <atomic>
#include <climits>
#include <mutex>

namespace kd {

static thread_local char g_err[512] = "";
char* err_buf() { return g_err; }

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

static std::atomic<bool> g_prof{false};
static std::mutex g_rec_mutex;            // launches may come from several host threads (one stream each): the record list is shared
static std::vector<ProfRec> g_recs;

bool prof_on() { return g_prof.load(std::memory_order_relaxed); }

static unsigned g_gen = 0;                // bumped by kd_prof_reset: a scope that began before a reset must not touch the records after it

ProfTicket prof_begin(const char* name, double flops, double bytes, hipStream_t s) {
  ProfRec r;
  r.name = name; r.flops = flops; r.bytes = bytes;
  (void)hipEventCreate(&r.e0);
  (void)hipEventCreate(&r.e1);
  (void)hipEventRecord(r.e0, s);
  std::lock_guard<std::mutex> lock(g_rec_mutex);
  g_recs.push_back(r);
  return ProfTicket{(int)g_recs.size() - 1, g_gen};
}

void prof_end(ProfTicket t, hipStream_t s) {
  // The end event is recorded UNDER the lock: kd_prof_reset destroys the events under the same lock, so the handle cannot die between
  // the look-up and the record.  A reset between begin and end changes the generation: index t.idx then names another launch's
  // record (or none) and is left alone.
  std::lock_guard<std::mutex> lock(g_rec_mutex);
  if (t.gen == g_gen && t.idx >= 0 && t.idx < (int)g_recs.size()) (void)hipEventRecord(g_recs[t.idx].e1, s);
}

}  // namespace kd

namespace kd {
int cu_count() {
  static std::atomic<int> cache[64];
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev < 0 || dev >= 64) dev = 0;
  int n = cache[dev].load(std::memory_order_relaxed);
  if (n <= 0) {
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cache[dev].store(n, std::memory_order_relaxed);
  }
  return n;
}
}  // namespace kd

using namespace kd;

// ---- library options (explicit switches instead of environment variables read inside the library) -------------------------
// include/kdiff_options.def is the table; the launch path reads g_opt through kd::opt (kd_common.h).  g_set only serves kd_get_option.
namespace kd {
#define KD_OPTION(name, dflt, doc) {dflt},
std::atomic<int> g_opt[KD_OPT_COUNT] = {
#include "../../include/kdiff_options.def"
};
#undef KD_OPTION
namespace {
#define KD_OPTION(name, dflt, doc) {#name, dflt},
const struct { const char* name; int dflt; } g_rows[KD_OPT_COUNT] = {
#include "../../include/kdiff_options.def"
};
#undef KD_OPTION
std::atomic<bool> g_set[KD_OPT_COUNT];
int option_index(const char* name) {
  for (int i = 0; i < KD_OPT_COUNT; ++i)
    if (!strcmp(g_rows[i].name, name)) return i;
  return -1;
}
}  // namespace
}  // namespace kd

extern "C" int kd_set_option(const char* name, int value) {
  if (!name) return fail(KD_EINVAL, "kd_set_option: null name");
  const int i = option_index(name);
  if (i < 0) return fail(KD_EINVAL, "kd_set_option: unknown option '%s'", name);
  g_set[i].store(value != INT_MIN, std::memory_order_relaxed);
  g_opt[i].store(value != INT_MIN ? value : g_rows[i].dflt, std::memory_order_relaxed);          // INT_MIN: back to the table's default
  return KD_OK;
}
// the caller-set value, else `dflt`; dflt == INT_MIN asks for the built-in default
extern "C" int kd_get_option(const char* name, int dflt) {
  const int i = name ? option_index(name) : -1;
  if (i < 0) return dflt;
  return g_set[i].load(std::memory_order_relaxed) || dflt == INT_MIN ? g_opt[i].load(std::memory_order_relaxed) : dflt;
}

extern "C" int kd_version(void) { return 200; }
extern "C" const char* kd_last_error(void) { return err_buf(); }

extern "C" int kd_prof_enable(int on) { g_prof.store(on != 0, std::memory_order_relaxed); return KD_OK; }
extern "C" int kd_prof_count(void) {
  std::lock_guard<std::mutex> lock(g_rec_mutex);
  return (int)g_recs.size();
}
extern "C" int kd_prof_get(int i, char* name, int name_cap, float* ms, double* flops, double* bytes) {
  ProfRec r;
  {
    std::lock_guard<std::mutex> lock(g_rec_mutex);
    if (i < 0 || i >= (int)g_recs.size()) return fail(KD_EINVAL, "kd_prof_get: index %d out of range", i);
    r = g_recs[i];
  }
  if (hipEventSynchronize(r.e1) != hipSuccess) return fail(KD_ELAUNCH, "kd_prof_get: event sync failed");
  float t = 0.f;
  if (hipEventElapsedTime(&t, r.e0, r.e1) != hipSuccess) return fail(KD_ELAUNCH, "kd_prof_get: elapsed failed");
  if (name && name_cap > 0) { strncpy(name, r.name.c_str(), name_cap - 1); name[name_cap - 1] = 0; }
  if (ms) *ms = t;
  if (flops) *flops = r.flops;
  if (bytes) *bytes = r.bytes;
  return KD_OK;
}
extern "C" int kd_prof_reset(void) {
  std::lock_guard<std::mutex> lock(g_rec_mutex);
  for (auto& r : g_recs) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
  g_recs.clear();
  ++g_gen;
  return KD_OK;
}
