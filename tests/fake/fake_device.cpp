// fake_device.cpp — TEST INFRASTRUCTURE: the device layer (flashgmm_amd/csrc/fgmm_device.h) and the kernel launchers
// (fgmm_internal.h) WITHOUT a GPU, so that the product's whole concurrent host pipeline - launch-unit planner, staging and pinned
// carve-up, the (bitstream, piece) task queue, event waits, overflow re-runs, the GPU-segment hand-back - runs on the CPU under
// ThreadSanitizer / AddressSanitizer (scripts/tsan_host.sh, tests/fake/stress_main.cpp).  Nothing here ships.
//
//   memory    "device" and "pinned" memory are host allocations
//   streams   every stream is an in-order queue run by its OWN thread; before each operation the thread may nap a random few
//             microseconds (FGMM_FAKE_JITTER_US): operations of different streams complete in shuffled order, those of one stream in
//             order - HIP's contract, and the only ordering the product may rely on
//   events    a counter pair (recorded, completed) under a mutex: the sanitizer sees exactly the happens-before edges the real
//             runtime gives (record -> everything before it on that stream; sync / stream_wait -> the record)
//   kernels   restated on the CPU from the oracle's float arithmetic (oracle/fgmm_oracle.c: fgo_symtab, fgo_cdftab, fgo_decode_gmm)
//             and the table format of fgmm_internal.h; float32 planes only, no fused softmax (the stress does not use them)
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#include "../../flashgmm_amd/csrc/fgmm_device.h"
#include "../../flashgmm_amd/csrc/fgmm_internal.h"

extern "C" {
void fgo_symtab(int mode, int64_t n, const int32_t *v, const float *scales, const float *means, const float *weights, int64_t sn, int64_t sk, uint32_t *packed);
void fgo_cdftab(int mode, int64_t n, const float *scales, const float *means, const float *weights, int64_t sn, int64_t sk, int32_t max_bs, uint16_t *tab);
int fgo_decode_gmm(int mode, const uint8_t *enc, size_t enc_len, int64_t n, const float *scales, const float *means, const float *weights, int64_t sn,
                   int64_t sk, int32_t max_bs, int32_t *out);
}

namespace fgmm {
namespace {

constexpr int kErrUnsupported = 801; // a kernel variant the fake does not restate

int jitter_us() {
  static const int v = getenv("FGMM_FAKE_JITTER_US") ? atoi(getenv("FGMM_FAKE_JITTER_US")) : 40;
  return v;
}

struct FakeStream {
  std::mutex m;
  std::condition_variable cv, idle_cv;
  std::deque<std::function<void()>> q;
  bool stop = false, busy = false;
  uint64_t rng;
  std::thread th;
  explicit FakeStream(uint64_t seed) : rng(seed * 0x9E3779B97F4A7C15ull + 1), th([this] { run(); }) {}
  ~FakeStream() {
    {
      std::lock_guard<std::mutex> l(m);
      stop = true;
    }
    cv.notify_all();
    th.join();
  }
  void push(std::function<void()> f) {
    {
      std::lock_guard<std::mutex> l(m);
      q.push_back(std::move(f));
    }
    cv.notify_one();
  }
  void sync() {
    std::unique_lock<std::mutex> l(m);
    idle_cv.wait(l, [this] { return q.empty() && !busy; });
  }
  void run() {
    for (;;) {
      std::function<void()> f;
      {
        std::unique_lock<std::mutex> l(m);
        cv.wait(l, [this] { return stop || !q.empty(); });
        if (q.empty()) return;
        f = std::move(q.front());
        q.pop_front();
        busy = true;
      }
      rng ^= rng << 13, rng ^= rng >> 7, rng ^= rng << 17;
      const int j = jitter_us();
      if (j > 0 && (rng & 3) == 0) std::this_thread::sleep_for(std::chrono::microseconds((rng >> 8) % (uint64_t)j));
      f();
      {
        std::lock_guard<std::mutex> l(m);
        busy = false;
      }
      idle_cv.notify_all();
    }
  }
};

struct FakeEvent {
  std::mutex m;
  std::condition_variable cv;
  uint64_t recorded = 0, completed = 0;
  std::chrono::steady_clock::time_point t;
};

std::atomic<uint64_t> g_stream_seed{1};
FakeStream *default_stream() {
  static FakeStream *s = new FakeStream(0); // (leaked on purpose: alive as long as any late call)
  return s;
}
FakeStream *S(dev::Stream s) { return s ? static_cast<FakeStream *>(s) : default_stream(); }

} // namespace

// ============================================================================================================== device layer
namespace dev {

int device_count(int *n) {
  *n = 1;
  return 0;
}
int get_device(int *d) {
  *d = 0;
  return 0;
}
int set_device(int d) { return d == 0 ? 0 : 101; }

int malloc_device(void **p, size_t bytes) {
  *p = malloc(bytes ? bytes : 1);
  return *p ? 0 : 2;
}
int free_device(void *p) {
  free(p);
  return 0;
}
int malloc_pinned(void **p, size_t bytes) { return malloc_device(p, bytes); }
int free_pinned(void *p) { return free_device(p); }
int mem_info(size_t *free_bytes, size_t *total_bytes) {
  static const size_t mb = getenv("FGMM_FAKE_MEM_MB") ? (size_t)atoll(getenv("FGMM_FAKE_MEM_MB")) : 2048;
  *free_bytes = *total_bytes = mb << 20;
  return 0;
}

int stream_create(Stream *s, bool) {
  *s = new FakeStream(g_stream_seed.fetch_add(1));
  return 0;
}
int stream_destroy(Stream s) {
  delete static_cast<FakeStream *>(s);
  return 0;
}
int stream_sync(Stream s) {
  S(s)->sync();
  return 0;
}
int event_create(Event *e, int) {
  *e = new FakeEvent;
  return 0;
}
int event_destroy(Event e) {
  delete static_cast<FakeEvent *>(e);
  return 0;
}
int event_record(Event e, Stream s) {
  FakeEvent *ev = static_cast<FakeEvent *>(e);
  uint64_t seq;
  {
    std::lock_guard<std::mutex> l(ev->m);
    seq = ++ev->recorded;
  }
  S(s)->push([ev, seq] {
    std::lock_guard<std::mutex> l(ev->m); // (notified under the lock: a waiter that returns may destroy the event at once)
    ev->completed = std::max(ev->completed, seq);
    ev->t = std::chrono::steady_clock::now();
    ev->cv.notify_all();
  });
  return 0;
}
int event_sync(Event e) { // the most recent record (none: returns at once)
  FakeEvent *ev = static_cast<FakeEvent *>(e);
  std::unique_lock<std::mutex> l(ev->m);
  const uint64_t want = ev->recorded;
  ev->cv.wait(l, [&] { return ev->completed >= want; });
  return 0;
}
int stream_wait_event(Stream s, Event e) {
  FakeEvent *ev = static_cast<FakeEvent *>(e);
  uint64_t want;
  {
    std::lock_guard<std::mutex> l(ev->m);
    want = ev->recorded;
  }
  S(s)->push([ev, want] {
    std::unique_lock<std::mutex> l(ev->m);
    ev->cv.wait(l, [&] { return ev->completed >= want; });
  });
  return 0;
}
int event_elapsed_ms(float *ms, Event a, Event b) {
  FakeEvent *ea = static_cast<FakeEvent *>(a), *eb = static_cast<FakeEvent *>(b);
  std::chrono::steady_clock::time_point ta, tb;
  {
    std::lock_guard<std::mutex> l(ea->m);
    ta = ea->t;
  }
  {
    std::lock_guard<std::mutex> l(eb->m);
    tb = eb->t;
  }
  *ms = std::chrono::duration<float, std::milli>(tb - ta).count();
  return 0;
}
int copy_async(void *dst, const void *src, size_t bytes, CopyKind, Stream s) {
  S(s)->push([dst, src, bytes] { memcpy(dst, src, bytes); });
  return 0;
}
int copy_sync(void *dst, const void *src, size_t bytes, CopyKind) { // (hipMemcpy: after everything on the default stream, complete on return)
  FakeStream *st = default_stream();
  st->push([dst, src, bytes] { memcpy(dst, src, bytes); });
  st->sync();
  return 0;
}
int memset_async(void *p, int value, size_t bytes, Stream s) {
  S(s)->push([p, value, bytes] { memset(p, value, bytes); });
  return 0;
}
const char *error_string(int e) { return e == kErrUnsupported ? "fake device: kernel variant not restated" : e == 2 ? "fake device: out of memory" : "fake device error"; }

} // namespace dev

// test-only hook (tests/fake/stress_main.cpp): a nap of `us` microseconds in the stream's queue - a producer that is still running when
// the call that consumes its output is made
extern "C" void fgmm_fake_delay(void *stream, int us) {
  S(stream)->push([us] { std::this_thread::sleep_for(std::chrono::microseconds(us)); });
}

// ================================================================================================================ the "kernels"
namespace {

inline float clamp_sigma(float s) { // entropy_models.py:817: torch.clamp keeps NaN, as clamp_scale does (fgmm_math.h); fminf / fmaxf would drop it
  s = (s < 0.11f) ? 0.11f : s;
  return (s > 256.0f) ? 256.0f : s;
}

// (hw, 4) rows of one channel of an item's planar parameters, sigma clamped when asked
struct Rows {
  std::vector<float> s, m, w;
  void gather(const void *scales, const void *means, const void *weights, int64_t stride_k, int64_t off_c, int64_t stride_p, int64_t hw, bool clamp) {
    s.resize((size_t)hw * 4), m.resize((size_t)hw * 4), w.resize((size_t)hw * 4);
    const float *S_ = static_cast<const float *>(scales), *M_ = static_cast<const float *>(means), *W_ = static_cast<const float *>(weights);
    for (int64_t p = 0; p < hw; ++p)
      for (int k = 0; k < 4; ++k) {
        const int64_t at = k * stride_k + off_c + p * stride_p;
        s[(size_t)p * 4 + k] = clamp ? clamp_sigma(S_[at]) : S_[at];
        m[(size_t)p * 4 + k] = M_[at];
        w[(size_t)p * 4 + k] = W_[at];
      }
  }
};

void k_quant_stats(const EncDesc *descs, int count) {
  for (int i = 0; i < count; ++i) {
    const EncDesc &d = descs[i];
    if (!d.chan_nz) continue; // (a raw-boundary item; a latent-layout item with M * hw == 0 may have a null y)
    int n_nz = 0;
    for (int c = 0; c < d.M; ++c) {
      float mn = INFINITY, mx = -INFINITY;
      int nz = 0;
      for (int64_t p = 0; p < d.hw; ++p) {
        const float v = d.y[(int64_t)c * d.hw + p], q = nearbyintf(v); // round-half-even (entropy_models.py:839)
        mn = fminf(mn, v), mx = fmaxf(mx, v);
        nz |= q != 0.0f;
        if (d.yq) d.yq[(int64_t)c * d.hw + p] = q;
      }
      d.chan_min[c] = mn, d.chan_max[c] = mx;
      if (d.chan_nz) d.chan_nz[c] = nz;
      if (d.chan_list && nz) d.chan_list[n_nz++] = c;
    }
    if (d.chan_list) d.chan_list[d.M] = n_nz;
  }
}

void k_symtab(const EncDesc *descs, int count, int mode, bool clamped) {
  Rows r;
  std::vector<int32_t> v;
  std::vector<uint32_t> packed;
  for (int i = 0; i < count; ++i) {
    const EncDesc &d = descs[i];
    const int n_ch = d.chan_list ? d.chan_list[d.M] : d.M;
    unsigned long long bypass = 0;
    for (int j = 0; j < n_ch; ++j) {
      const int c = d.chan_list ? d.chan_list[j] : j;
      r.gather(d.scales, d.means, d.weights, d.stride_k, (int64_t)c * d.stride_c, d.stride_p, d.hw, clamped);
      v.resize((size_t)d.hw), packed.resize((size_t)d.hw);
      for (int64_t p = 0; p < d.hw; ++p) v[(size_t)p] = d.y ? (int32_t)nearbyintf(d.y[(int64_t)c * d.hw + p]) : d.sym[p];
      fgo_symtab(mode, d.hw, v.data(), r.s.data(), r.m.data(), r.w.data(), 4, 1, packed.data());
      uint32_t *out;
      if (d.seg_b[0] == INT32_MAX) out = d.packed + (int64_t)j * d.hw;
      else {
        const int s = (j >= d.seg_b[0]) + (j >= d.seg_b[1]) + (j >= d.seg_b[2]);
        out = d.packed_seg[s] + (int64_t)(j - s * d.cps) * d.hw;
      }
      for (int64_t p = 0; p < d.hw; ++p) {
        out[p] = packed[(size_t)p];
        bypass += (packed[(size_t)p] >> 16) == 0;
      }
    }
    if (d.meta) d.meta[0] += (uint32_t)bypass;
  }
}

// a trimmed row: F_i[a .. a + cnt) from the first non-zero edge to the start of the trailing constant run (tests/helpers.py:_trim_row)
struct Trim {
  int64_t a_idx, cnt;
  uint32_t nonmono;
};
Trim trim_row(const uint16_t *F, int64_t W) {
  int64_t first_nz = W;
  for (int64_t j = 0; j < W; ++j)
    if (F[j]) {
      first_nz = j;
      break;
    }
  const int64_t lead = first_nz < W ? first_nz - 1 : W - 1;
  int64_t run_start = 0;
  for (int64_t j = W - 1; j >= 0; --j)
    if (F[j] != F[W - 1]) {
      run_start = j + 1;
      break;
    }
  Trim t;
  t.a_idx = std::min(lead + 1, run_start);
  t.cnt = run_start - t.a_idx + 1;
  t.nonmono = 0;
  for (int64_t j = t.a_idx + 1; j < t.a_idx + t.cnt; ++j) t.nonmono |= F[j] < F[j - 1];
  return t;
}
// the row's bytes (raw uint16 entries or the Elias-Fano bit string), appended to `out`
void row_payload(const uint16_t *row, uint32_t cnt, uint32_t nonmono, uint32_t ef_min, std::vector<uint8_t> &out) {
  const size_t at = out.size();
  const size_t nb = (size_t)tab_row_bytes(cnt, nonmono, ef_min);
  out.resize(at + nb, 0);
  uint8_t *o = out.data() + at;
  if (!tab_row_is_ef(cnt, nonmono, ef_min)) {
    memcpy(o, row, 2 * (size_t)cnt);
    return;
  }
  const uint32_t l = tab_ef_l(cnt), LB = tab_ef_lb(cnt, l);
  auto set_bit = [o](uint64_t b) { o[b >> 3] |= (uint8_t)(1u << (b & 7)); };
  for (uint32_t j = 0; j < cnt; ++j) {
    set_bit((uint64_t)(row[j] >> l) + j);
    for (uint32_t b = 0; b < l; ++b)
      if ((row[j] >> b) & 1u) set_bit((uint64_t)LB + (uint64_t)j * l + b);
  }
}

// headers + rows of latents [lat0, lat1) of an item (compact order), rows appended to `rows` in latent order; hdr_form 2 / 4 / 8
void build_rows(const DecDesc &d, int mode, bool clamped, int64_t lat0, int64_t lat1, uint8_t *hdr_out, int hdr_form, std::vector<uint8_t> &rows, bool *any_nonmono) {
  const int64_t W = 2 * (int64_t)d.max_bs + 2;
  Rows r;
  std::vector<uint16_t> F((size_t)W);
  int64_t cur_c = -1;
  for (int64_t i = lat0; i < lat1; ++i) {
    const int64_t j = i / d.hw, p = i - j * d.hw;
    if (j != cur_c) {
      const int c = d.chan_list ? d.chan_list[j] : (int)j;
      r.gather(d.scales, d.means, d.weights, d.stride_k, (int64_t)c * d.stride_c, d.stride_p, d.hw, clamped);
      cur_c = j;
    }
    fgo_cdftab(mode, 1, r.s.data() + 4 * p, r.m.data() + 4 * p, r.w.data() + 4 * p, 4, 1, d.max_bs, F.data());
    const Trim t = trim_row(F.data(), W);
    const int32_t a = (int32_t)(t.a_idx - d.max_bs);
    *any_nonmono |= t.nonmono != 0;
    uint8_t *h = hdr_out + (size_t)hdr_form * (size_t)(i - lat0);
    if (hdr_form == 2) {
      const uint16_t v = (uint16_t)(t.a_idx | ((t.nonmono ? kHdr2Escape : (uint32_t)t.cnt) << 8));
      memcpy(h, &v, 2);
      if (t.nonmono) { // the row begins with a 4-byte header of the next form
        const uint32_t h4 = tab_hdr_pack(a, (uint32_t)t.cnt, 1);
        const uint8_t *b = reinterpret_cast<const uint8_t *>(&h4);
        rows.insert(rows.end(), b, b + 4);
      }
    } else if (hdr_form == 4) {
      const uint32_t v = tab_hdr_pack(a, (uint32_t)t.cnt, t.nonmono);
      memcpy(h, &v, 4);
    } else {
      const unsigned long long v = tab_hdr8_pack(a, (uint32_t)t.cnt, t.nonmono);
      memcpy(h, &v, 8);
    }
    row_payload(F.data() + t.a_idx, (uint32_t)t.cnt, t.nonmono, d.ef_min, rows);
  }
}

std::mutex g_cursor_mu; // the launch's cursor is ONE atomic on the device; here the blocks of a launch are placed under a lock

// single-pass table kernel: the blocks [blk_begin, blk_end) of every part, each block's rows at the launch's cursor (blocks in a
// shuffled order: the real kernel places them in arrival order)
void k_tab(const DecDesc *descs, int count, int mode, bool clamped, uint64_t shuffle) {
  for (int q = 0; q < count; ++q) {
    const DecDesc &d = descs[q];
    if (getenv("FGMM_FAKE_VERBOSE"))
      fprintf(stderr, "   [k_tab] part %d/%d: n %lld hw %lld n_ch %d tl %d blocks [%d, %d) max_bs %d hdr_form %d stride k %lld c %lld p %lld\n", q, count, (long long)d.n,
              (long long)d.hw, d.n_ch, d.tl, d.blk_begin, d.blk_end, d.max_bs, d.hdr_form, (long long)d.stride_k, (long long)d.stride_c, (long long)d.stride_p);
    std::vector<int32_t> order;
    for (int32_t b = d.blk_begin; b < d.blk_end; ++b) order.push_back(b);
    for (size_t k = order.size(); k > 1; --k) {
      shuffle ^= shuffle << 13, shuffle ^= shuffle >> 7, shuffle ^= shuffle << 17;
      std::swap(order[k - 1], order[shuffle % k]);
    }
    std::vector<uint8_t> rows;
    for (int32_t b : order) {
      const int64_t lat0 = std::min<int64_t>((int64_t)b * d.tl, d.n), lat1 = std::min<int64_t>((int64_t)(b + 1) * d.tl, d.n);
      rows.clear();
      bool nonmono = false;
      uint8_t *hdr = static_cast<uint8_t *>(d.hdr_out) + (size_t)d.hdr_form * (size_t)(lat0 - std::min<int64_t>((int64_t)d.blk_begin * d.tl, d.n));
      build_rows(d, mode, clamped, lat0, lat1, hdr, d.hdr_form, rows, &nonmono);
      const unsigned long long B4 = (rows.size() + 3ull) & ~3ull;
      std::lock_guard<std::mutex> l(g_cursor_mu);
      const unsigned long long base = d.counters[0];
      d.counters[0] += B4;
      if (nonmono) d.counters[3] += 1;
      if (d.count_edges) d.counters[4 + (b & (kTabEdgeSlots - 1))] += (unsigned long long)(lat1 - lat0) * (unsigned long long)(2 * (int64_t)d.max_bs + 2);
      d.blkoff_out[b - d.blk_begin] = (uint32_t)(base >> 2);
      if (base + B4 > d.rows_cap) {
        d.counters[1] |= 1ull;
        continue;
      }
      memcpy(d.rows + base, rows.data(), rows.size());
      memset(d.rows + base + rows.size(), 0, (size_t)(B4 - rows.size()));
    }
  }
}

// generic two-pass kernels: 4- or 8-byte headers, rows sequential in latent order.  pass 1 (count): headers + pool_used[0] = bytes;
// pass 2 (fill): the rows into d.pool
void k_cdftab(const DecDesc *descs, int count, int mode, bool clamped, int pass) {
  for (int q = 0; q < count; ++q) {
    const DecDesc &d = descs[q];
    const int form = d.hdr_form == 8 ? 8 : 4;
    std::vector<uint8_t> rows, hdr((size_t)form * (size_t)std::max<int64_t>(d.n, 1));
    bool nonmono = false;
    if (2 * (int64_t)d.max_bs + 2 > (1 << 20)) { // (the real kernels prune the saturated tails first; the fake refuses what it would not evaluate)
      d.pool_used[3] = 1;
      continue;
    }
    build_rows(d, mode, clamped, 0, d.n, hdr.data(), form, rows, &nonmono);
    if (pass & 1) {
      memcpy(d.hdr, hdr.data(), (size_t)form * (size_t)d.n);
      d.pool_used[0] = rows.size();
      d.pool_used[2] = nonmono;
    }
    if (pass & 2) {
      if (rows.size() > d.pool_cap) d.pool_used[1] = 1;
      else if (d.pool) memcpy(d.pool, rows.data(), rows.size());
    }
  }
}

void k_segzero(const SegDesc *descs, int count) {
  for (int i = 0; i < count; ++i)
    for (int64_t k = 0; k < descs[i].n_dead; ++k) {
      float *o = descs[i].y_hat + (int64_t)descs[i].dead_list[k] * descs[i].hw;
      for (int64_t p = 0; p < descs[i].hw; ++p) o[p] = 0.0f;
    }
}
// the GPU's segment decoder, restated crudely: every OTHER item is decoded (whole, by the oracle's float bisection) and reported
// verified, the rest is reported as not settled - so that both the "decoded on the GPU" and the "handed back to the table path"
// branches of the orchestration run
void k_segdec(const SegDesc *descs, const SegRef *segs, int64_t n_segs, int mode, bool clamped) {
  int n_items = 0;
  for (int64_t s = 0; s < n_segs; ++s) n_items = std::max(n_items, segs[s].item + 1);
  for (int i = 0; i < n_items; ++i) {
    const SegDesc &d = descs[i];
    bool ok = (i & 1) == 0;
    if (ok) {
      const int64_t n_ch = d.hw ? d.n / d.hw : 0;
      std::vector<float> s((size_t)d.n * 4), m((size_t)d.n * 4), w((size_t)d.n * 4);
      Rows r;
      for (int64_t j = 0; j < n_ch; ++j) {
        r.gather(d.scales, d.means, d.weights, d.stride_k, (int64_t)d.chan_list[j] * d.stride_c, d.stride_p, d.hw, clamped);
        memcpy(s.data() + 4 * j * d.hw, r.s.data(), sizeof(float) * 4 * (size_t)d.hw);
        memcpy(m.data() + 4 * j * d.hw, r.m.data(), sizeof(float) * 4 * (size_t)d.hw);
        memcpy(w.data() + 4 * j * d.hw, r.w.data(), sizeof(float) * 4 * (size_t)d.hw);
      }
      std::vector<int32_t> out((size_t)std::max<int64_t>(d.n, 1));
      ok = fgo_decode_gmm(mode, reinterpret_cast<const uint8_t *>(d.words), (size_t)d.n_words * 4, d.n, s.data(), m.data(), w.data(), 4, 1, d.max_bs, out.data()) == 0;
      if (ok)
        for (int64_t j = 0; j < n_ch; ++j)
          for (int64_t p = 0; p < d.hw; ++p) d.y_hat[(int64_t)d.chan_list[j] * d.hw + p] = (float)out[(size_t)(j * d.hw + p)];
    }
    for (int64_t sg = 0; sg <= d.n_ckpt; ++sg) d.status[sg] = ok ? kSegOk : kSegHard;
  }
}

void k_scatter_round(const ScatDesc *descs, int count, int round) {
  for (int i = 0; i < count; ++i) {
    const ScatDesc &d = descs[i];
    if (!d.y_hat) continue;
    for (int64_t k = d.bound[round]; k < d.bound[round + 1]; ++k) {
      const int64_t r = k / d.hw;
      d.y_hat[(int64_t)d.chan_list[r] * d.hw + (k - r * d.hw)] = (float)d.sym[k];
    }
  }
}

std::atomic<uint64_t> g_launch{0x1234567ull};

} // namespace

// ================================================================================================================ the launchers
int launch_quant_stats(const EncDesc *d, int count, int, void *stream) {
  S(stream)->push([d, count] { k_quant_stats(d, count); });
  return 0;
}
int launch_symtab(const EncDesc *d, int count, int, int64_t, int64_t, bool, int mode, int, bool clamped, bool f16, void *stream) {
  if (f16) return kErrUnsupported;
  S(stream)->push([d, count, mode, clamped] { k_symtab(d, count, mode, clamped); });
  return 0;
}
int launch_tab(const DecDesc *d, int count, int, int, int, int mode, bool clamped, bool f16, void *stream) {
  if (f16) return kErrUnsupported;
  const uint64_t sh = g_launch.fetch_add(0x9E3779B97F4A7C15ull);
  S(stream)->push([d, count, mode, clamped, sh] { k_tab(d, count, mode, clamped, sh | 1); });
  return 0;
}
int launch_cdftab_count(const DecDesc *d, int count, int, int64_t, int mode, bool clamped, bool f16, void *stream) {
  if (f16) return kErrUnsupported;
  S(stream)->push([d, count, mode, clamped] { k_cdftab(d, count, mode, clamped, 1); });
  return 0;
}
int launch_cdftab_fill(const DecDesc *d, int count, int, int64_t, int mode, bool clamped, bool f16, void *stream) {
  if (f16) return kErrUnsupported;
  S(stream)->push([d, count, mode, clamped] { k_cdftab(d, count, mode, clamped, 2); });
  return 0;
}
int launch_cdftab(const DecDesc *d, int count, int, int64_t, int mode, bool clamped, bool f16, void *stream) {
  if (f16) return kErrUnsupported;
  S(stream)->push([d, count, mode, clamped] { k_cdftab(d, count, mode, clamped, 3); });
  return 0;
}
int launch_yhat_scatter(const void *sym, int wide, const int32_t *rank, float *y_hat, int M, int64_t hw, void *stream) {
  S(stream)->push([=] {
    for (int c = 0; c < M; ++c)
      for (int64_t p = 0; p < hw; ++p) {
        const int r = rank[c];
        y_hat[(int64_t)c * hw + p] = r < 0 ? 0.0f : wide ? (float)static_cast<const int32_t *>(sym)[(int64_t)r * hw + p] : (float)static_cast<const int16_t *>(sym)[(int64_t)r * hw + p];
      }
  });
  return 0;
}
int launch_yhat_scatter_round(const ScatDesc *d, int count, int round, int64_t max_range, void *stream) {
  if (count <= 0 || max_range <= 0) return 0;
  S(stream)->push([d, count, round] { k_scatter_round(d, count, round); });
  return 0;
}
int launch_yhat_zero_dead(const ScatDesc *d, int count, int, int64_t, void *stream) {
  S(stream)->push([d, count] {
    for (int i = 0; i < count; ++i)
      if (d[i].y_hat)
        for (int c = 0; c < d[i].M; ++c)
          if (d[i].rank[c] < 0)
            for (int64_t p = 0; p < d[i].hw; ++p) d[i].y_hat[(int64_t)c * d[i].hw + p] = 0.0f;
  });
  return 0;
}
int launch_segzero(const SegDesc *d, int count, int64_t max_dead, void *stream) {
  if (count <= 0 || max_dead <= 0) return 0;
  S(stream)->push([d, count] { k_segzero(d, count); });
  return 0;
}
int launch_segdec(const SegDesc *d, const SegRef *segs, int64_t n_segs, int mode, bool clamped, bool f16, void *stream) {
  if (n_segs <= 0) return 0;
  if (f16) return kErrUnsupported;
  S(stream)->push([d, segs, n_segs, mode, clamped] { k_segdec(d, segs, n_segs, mode, clamped); });
  return 0;
}
// probes and self-tests of the real kernels' arithmetic: nothing of the host pipeline to exercise
int launch_cdf_pair(const int32_t *, const float *, const float *, const float *, int64_t, int64_t, int64_t, int, float *, float *, void *) { return kErrUnsupported; }
int launch_softmax_probe(const float *, float *, int64_t, void *) { return kErrUnsupported; }
// the parameter head (fgmm_head.hip) is a kernel in front of the SAME host pipeline (fgmm_encode.cpp takes its table from it instead of
// symtab_kernel's): not restated here - its arithmetic is pinned on the GPU against oracle/fgmm_oracle.c fgo_head_params
int launch_head_pack(const float *, const float *, int, int, float *, float *, void *) { return kErrUnsupported; }
size_t head16_packed_bytes(int, int) { return 16; }
size_t head16_split_elems(int, int64_t) { return 0; }
int launch_head16_split(const float *, void *, int64_t, int, int, int64_t, int64_t, void *) { return kErrUnsupported; }
int launch_head16_pack(const float *, const float *, int, int, void *, void *) { return kErrUnsupported; }
int launch_head16_params(const HeadDesc *, const HeadW &, int, int64_t, void *) { return kErrUnsupported; }
int launch_head16_symtab(const EncDesc *, const HeadW &, int, int, int64_t, int, bool, void *) { return kErrUnsupported; }
int launch_head_params(const HeadDesc *, const HeadW &, int, int64_t, bool, void *) { return kErrUnsupported; }
int launch_head_symtab(const EncDesc *, const HeadW &, int, int, int64_t, int, bool, bool, void *) { return kErrUnsupported; }
int launch_ckbd(const void *, void *, int64_t, int64_t, int64_t, int, int, bool, void *) { return kErrUnsupported; }
int launch_fastmath_selftest(int, unsigned long long, unsigned long long, unsigned long long *, void *) { return kErrUnsupported; }
int launch_saturation_selftest(int, unsigned long long *, void *) { return kErrUnsupported; }

} // namespace fgmm
