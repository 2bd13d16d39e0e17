// rtc_rowtable.h -- the row kernels that score "the groups next to a vertex", written once.  The rules are move_rule and
// place_rule (rtc_community.h) and sil_rule (rtc_quality.hip).
//   device  RowTable    an open-addressing table keyed by a group id, in LDS or in global memory: clear, claim, find, read
//           row_reduce  a value folded over the workgroup: xor shuffles, one LDS slot a wave, lane 0 folds the waves
//           row_kernel  one row a workgroup and turn -- clear | gather | sweep, reduce, lane 0 writes | -- as a template over a rule
//   host    RowPaths    the rows by kernel path (by length alone), the tables of the long ones, and the three launches
// A table always has two slots or more per entry of its row, so a probe ends.  Everything is in integers and order-free.
#ifndef RTC_ROWTABLE_H
#define RTC_ROWTABLE_H
#include "rtc_internal.h"

namespace {

constexpr uint32_t RT_NONE = 0xffffffffu;  // the key of a free slot; find's "not there"

// The table of one row.  CNT: a slot holds a count beside its sum (16 bytes a slot, else 12).
// AGENT_READS says how a slot of a global table is read after the gather.  The slots were written by this workgroup's atomics,
// which act in L2.  true: the read goes there too (device scope) and never takes a line that the CU's vector cache kept from
// before.  false: a plain load.  Both are right: every long row has a table of its own, which no other workgroup touches during
// the launch and which this workgroup does not load from before the barrier behind its gather.  Each rule keeps the kind of read
// its kernel was written and measured with.  LDS slots are always read plainly.
template <bool CNT, bool AGENT_READS>
struct RowTable {
  uint32_t *keys, *cnt;
  unsigned long long* sum;
  uint32_t slots, mask, shift;
  bool global;  // a constant once open<SLOTS> is inlined

  // SLOTS > 0: the kernel's LDS arrays.  SLOTS == 0: 1 << tab_log2[it] slots from tab_off[it] on in the launch's global arrays;
  // the two lists are NULL otherwise and are not touched.
  template <uint32_t SLOTS>
  static __device__ __forceinline__ RowTable open(uint32_t* keys, uint32_t* cnt, unsigned long long* sum, const uint64_t* tab_off,
                                                  const uint32_t* tab_log2, uint32_t it) {
    const uint32_t log2_slots = SLOTS ? 31 - __builtin_clz(SLOTS ? SLOTS : 1u) : tab_log2[it];
    const uint64_t off = SLOTS ? 0 : tab_off[it];
    return RowTable{keys + off, CNT ? cnt + off : cnt, sum + off, 1u << log2_slots, (1u << log2_slots) - 1, 32 - log2_slots, SLOTS == 0};
  }
  template <int BLOCK>
  __device__ __forceinline__ void clear() const {
    for (uint32_t s = threadIdx.x; s < slots; s += BLOCK) { keys[s] = RT_NONE; if (CNT) cnt[s] = 0u; sum[s] = 0ull; }
  }
  // group d's slot, claimed if it had none; the caller adds to sum[slot] and cnt[slot]
  __device__ __forceinline__ uint32_t claim(uint32_t d) const {
    uint32_t h = (d * 2654435761u) >> shift;
    for (;;) {
      const uint32_t old = atomicCAS(&keys[h], RT_NONE, d);
      if (old == RT_NONE || old == d) return h;
      h = (h + 1) & mask;
    }
  }
  template <class T>
  __device__ __forceinline__ T read(const T* p) const {
    return AGENT_READS && global ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : *p;
  }
  // after the gather: group d's slot, RT_NONE if it has none
  __device__ __forceinline__ uint32_t find(uint32_t d) const {
    for (uint32_t h = (d * 2654435761u) >> shift;; h = (h + 1) & mask) {
      const uint32_t k = read(&keys[h]);
      if (k == d || k == RT_NONE) return k == d ? h : RT_NONE;
    }
  }
};

// lane ^ off's v.  V is whole 32-bit words without padding (a struct is packed: its wave slots are LDS, which must not grow)
template <class V>
__device__ __forceinline__ V row_shfl_xor(const V& v, int off) {
  static_assert(sizeof(V) % 4 == 0, "whole words");
  uint32_t word[sizeof(V) / 4];
  __builtin_memcpy(word, &v, sizeof(V));
#pragma unroll
  for (uint32_t i = 0; i < sizeof(V) / 4; i++) word[i] = __shfl_xor(word[i], off);
  V o;
  __builtin_memcpy(&o, word, sizeof(V));
  return o;
}
// The workgroup's fold, in two steps so that a rule can put the kernel's barrier between them.  fold(mine, other) folds other
// into mine: a "best" under an order keeps the better one, a top two or a sum keeps more.
// Every lane of a wave gets the wave's fold, and lane 0 leaves it in lds[wave].
template <int BLOCK, class V, class Fold>
__device__ __forceinline__ V row_reduce_wave(V v, Fold fold, V* lds) {
  for (int off = 32; off; off >>= 1) fold(v, row_shfl_xor(v, off));
  if (BLOCK > 64 && (threadIdx.x & 63) == 0) lds[threadIdx.x / 64] = v;
  return v;
}
// behind a barrier: the workgroup's fold, for every lane that asks
template <int BLOCK, class V, class Fold>
__device__ __forceinline__ V row_reduce_all(V v, Fold fold, const V* lds) {
  if (BLOCK > 64) {
    v = lds[0];
    for (uint32_t wv = 1; wv < BLOCK / 64; wv++) fold(v, lds[wv]);
  }
  return v;
}
// both, with a barrier of its own where there is more than one wave: lane 0 gets the workgroup's fold
template <int BLOCK, class V, class Fold>
__device__ __forceinline__ V row_reduce(V v, Fold fold, V* lds) {
  v = row_reduce_wave<BLOCK>(v, fold, lds);
  if (BLOCK > 64) __syncthreads();
  return threadIdx.x == 0 ? row_reduce_all<BLOCK>(v, fold, lds) : v;
}

// Row list[it], one a workgroup and turn.  A rule is the row's state in registers and gives
//   Args, Best, Lds, Table    its kernel arguments (with row_off), what the sweep reduces, its wave slots (Lds::best[4]), its RowTable
//   shape                     the paths' sizes (RowPaths below)
//   enter(a, x)               false: the row is skipped, before the clear.  Uniform, because x is
//   gather(a, tab, x, e)      entry e of the row: claim and add
//   gathered<BLOCK>(lds)      row_reduce_wave of what was reduced beside the gather, in front of the barrier that ends the gather
//   begin<BLOCK>(a, tab, x, lds)  behind that barrier: the row's own terms; returns the lane's first Best
//   sweep(a, tab, s, best)    slot s of the table
//   fold(best, other)         the order
//   finish(a, tab, x, len, best)  lane 0 alone: the row's result
// The barriers are reached by all: the loop and enter are uniform over the workgroup.
template <int BLOCK, uint32_t SLOTS, class Rule>
__global__ __launch_bounds__(BLOCK) void row_kernel(const uint32_t* __restrict__ list, uint32_t n_list, const uint64_t* __restrict__ tab_off,
                                                    const uint32_t* __restrict__ tab_log2, uint32_t* gkeys, uint32_t* gcnt,
                                                    unsigned long long* gsum, typename Rule::Args a) {
  __shared__ uint32_t s_keys[SLOTS ? SLOTS : 1];
  __shared__ uint32_t s_cnt[SLOTS && Rule::shape::CNT ? SLOTS : 1];
  __shared__ unsigned long long s_sum[SLOTS ? SLOTS : 1];
  __shared__ typename Rule::Lds lds;
  for (uint32_t it = blockIdx.x; it < n_list; it += gridDim.x) {
    const uint32_t x = list[it];
    Rule r;
    if (!r.enter(a, x)) continue;
    const typename Rule::Table tab =
        Rule::Table::template open<SLOTS>(SLOTS ? s_keys : gkeys, SLOTS ? s_cnt : gcnt, SLOTS ? s_sum : gsum, tab_off, tab_log2, it);
    tab.template clear<BLOCK>();
    __syncthreads();
    const uint64_t r0 = a.row_off[x], r1 = a.row_off[x + 1];
    for (uint64_t e = r0 + threadIdx.x; e < r1; e += BLOCK) r.gather(a, tab, x, e);
    r.template gathered<BLOCK>(lds);
    __syncthreads();  // the table is complete, and so is what the waves reduced beside it
    typename Rule::Best best = r.template begin<BLOCK>(a, tab, x, lds);
    for (uint32_t s = threadIdx.x; s < tab.slots; s += BLOCK) r.sweep(a, tab, s, best);
    best = row_reduce<BLOCK>(best, Rule::fold, lds.best);
    if (threadIdx.x == 0) r.finish(a, tab, x, r1 - r0, best);
    __syncthreads();  // the table and the wave slots are written again in the next turn
  }
}

// The rows of a CSR by kernel path (which one a row takes depends on its length alone) and the tables of the long ones.
// Shape: WAVE_ROW / WAVE_SLOTS (one wave, the table in LDS), BLOCK_ROW / BLOCK_SLOTS (256 lanes, LDS), GLOBAL_LOG2_MIN (longer
// rows: 256 lanes, a table of 1 << max(that, ceil(log2(2 L))) slots in global memory), WGS_PER_CU[3] (the grid of each path,
// at most one workgroup a row) and CNT.
template <class Shape>
struct RowPaths {
  std::vector<uint64_t> h_row, h_off;
  std::vector<uint32_t> lists[3], h_log2;
  uint64_t table_slots = 0;
  uint32_t *d_list[3] = {nullptr, nullptr, nullptr}, *d_log2 = nullptr, *d_gkeys = nullptr, *d_gcnt = nullptr;
  uint64_t* d_off = nullptr;
  unsigned long long* d_gsum = nullptr;

  // the row offsets of nl rows, on the host; synchronises the stream
  int fetch(rtc_ctx* ctx, const uint64_t* d_row_off, uint32_t nl) {
    h_row.resize((size_t)nl + 1);
    RTC_HIP(ctx, hipMemcpyAsync(h_row.data(), d_row_off, ((size_t)nl + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    RTC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RTC_OK;
  }
  // The lists, from the fetched offsets.  A row without an entry, or with keep(x) false, is on none.  all_global: every listed
  // row takes the global path.
  template <class Keep>
  int plan(rtc_ctx* ctx, const char* who, bool all_global, Keep keep) {
    for (auto* l : {&lists[0], &lists[1], &lists[2], &h_log2}) l->clear();
    h_off.clear();
    table_slots = 0;
    for (uint32_t x = 0; x + 1 < h_row.size(); x++) {
      const uint64_t len = h_row[x + 1] - h_row[x];
      if (len == 0 || !keep(x)) continue;
      if (!all_global && len <= Shape::WAVE_ROW) lists[0].push_back(x);
      else if (!all_global && len <= Shape::BLOCK_ROW) lists[1].push_back(x);
      else {
        uint32_t lg = Shape::GLOBAL_LOG2_MIN;
        while ((1ull << lg) < 2 * len) lg++;
        if (lg > 31) return rtc_fail(ctx, RTC_ERR_UNSUPPORTED, "%s: a row of %llu entries", who, (unsigned long long)len);
        lists[2].push_back(x);
        h_log2.push_back(lg);
        h_off.push_back(table_slots);
        table_slots += 1ull << lg;
      }
    }
    return RTC_OK;
  }
  // what alloc will ask for: the lists (4 bytes a row), the tables, and 12 bytes a long row for where its table is and how large
  uint64_t bytes() const {
    return 4ull * (lists[0].size() + lists[1].size() + lists[2].size()) + (Shape::CNT ? 16 : 12) * table_slots + 12ull * lists[2].size();
  }
  int path_mask() const { return (lists[0].empty() ? 0 : 1) | (lists[1].empty() ? 0 : 2) | (lists[2].empty() ? 0 : 4); }
  // the copies are only enqueued: the host lists stay as they are until the stream is synchronised
  int alloc(rtc_ctx* ctx, DevBuf& db) {
    for (int p = 0; p < 3; p++)
      if (!lists[p].empty()) {
        RTC_TRY(db.get(ctx, lists[p].size(), &d_list[p]));
        RTC_HIP(ctx, hipMemcpyAsync(d_list[p], lists[p].data(), lists[p].size() * 4, hipMemcpyHostToDevice, ctx->stream));
      }
    if (lists[2].empty()) return RTC_OK;
    RTC_TRY(db.get(ctx, h_log2.size(), &d_log2));
    RTC_TRY(db.get(ctx, h_off.size(), &d_off));
    RTC_TRY(db.get(ctx, table_slots, &d_gkeys));
    if (Shape::CNT) RTC_TRY(db.get(ctx, table_slots, &d_gcnt));
    RTC_TRY(db.get(ctx, table_slots, &d_gsum));
    RTC_HIP(ctx, hipMemcpyAsync(d_log2, h_log2.data(), h_log2.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    RTC_HIP(ctx, hipMemcpyAsync(d_off, h_off.data(), h_off.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    return RTC_OK;
  }
  // Every row with an entry, by its length, without asking whether the memory is there.  Synchronises the stream: the host
  // lists are rewritten at the next level.
  int prepare(rtc_ctx* ctx, DevBuf& db, const uint64_t* d_row_off, uint32_t nl, const char* who) {
    RTC_TRY(fetch(ctx, d_row_off, nl));
    RTC_TRY(plan(ctx, who, false, [](uint32_t) { return true; }));
    RTC_TRY(alloc(ctx, db));
    RTC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RTC_OK;
  }
  void release(DevBuf& db) {
    for (void** q : {(void**)&d_list[0], (void**)&d_list[1], (void**)&d_list[2], (void**)&d_log2, (void**)&d_off, (void**)&d_gkeys, (void**)&d_gcnt,
                     (void**)&d_gsum})
      if (*q) { db.release(*q); *q = nullptr; }
  }

  // one pass over every listed row: a launch a path; only the global path reads the table arguments
  template <class Rule>
  int launch(rtc_ctx* ctx, const typename Rule::Args& a) {
    static_assert(std::is_same<typename Rule::shape, Shape>::value, "the rule's shape");
    auto path = [&](auto kernel, uint32_t block, int p) -> int {
      if (lists[p].empty()) return RTC_OK;
      const uint32_t nb = (uint32_t)std::min<uint64_t>(lists[p].size(), (uint64_t)ctx->num_cu * Shape::WGS_PER_CU[p]);
      hipLaunchKernelGGL(kernel, dim3(nb), dim3(block), 0, ctx->stream, (const uint32_t*)d_list[p], (uint32_t)lists[p].size(),
                         (const uint64_t*)d_off, (const uint32_t*)d_log2, d_gkeys, d_gcnt, d_gsum, a);
      RTC_CHECK_LAUNCH(ctx);
      return RTC_OK;
    };
    RTC_TRY(path(row_kernel<64, Shape::WAVE_SLOTS, Rule>, 64, 0));
    RTC_TRY(path(row_kernel<256, Shape::BLOCK_SLOTS, Rule>, 256, 1));
    return path(row_kernel<256, 0, Rule>, 256, 2);
  }
};

}  // namespace

#endif  // RTC_ROWTABLE_H
