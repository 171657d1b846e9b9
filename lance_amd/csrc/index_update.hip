// index_update.hip -- index maintenance on the device: merge (append), remap / delete, and the row-major read side.
//
//   optimize_indices / merge of deltas   rust/lance/src/index/vector/ivf.rs:355-560, builder.rs:685-935 (take_partition_batches)
//   remap(HashMap<u64, Option<u64>>)      builder.rs:256-359, pq/storage.rs:499-560, quantizer.rs:244-280
//   to_batches                            the stored rows, row-major
// Every operation builds a NEW handle (fresh serial: captured searches of the sources stay valid) and never writes a source.  The
// payload -- PQ codes, IVF_FLAT vectors, SQ codes + their sums, row ids -- moves HBM -> HBM through one copy kernel; only the
// partition offsets (at most 65,537 words per handle, already mirrored on the host) are computed on the host.
// What is built here is the reference's no-split / no-join branch: partitions are neither split on append nor joined on remap
// (rebalance.hip: lance_hip_index_split / _join, built from the pieces below).
#include <algorithm>
#include <vector>

#include "common.h"
#include "index.h"
#include "kernels.h"

namespace lh {

// ---- device code (plain index arithmetic, loads and stores: tests/test_index_update_kernels_cpu.py runs this text on the CPU)
constexpr uint32_t IU_NONE = 0xFFFFFFFFu;             // LANCE_HIP_NONE
constexpr uint64_t IU_DELETED = 0xFFFFFFFFFFFFFFFFull;   // LANCE_HIP_ROW_DELETED

// largest p in [0, nlist) with offs[p] <= row: the partition of stored row `row` (row < offs[nlist]; empty partitions are skipped)
__device__ __forceinline__ uint32_t iu_partition_of(const uint32_t *__restrict__ offs, int nlist, uint32_t row) {
  int lo = 0, hi = nlist;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (offs[mid] <= row) lo = mid; else hi = mid;
  }
  return (uint32_t)lo;
}

// One per-row array on the move.  Three forms, by which pointers are set:
//   perm                 gather:  destination row r takes source row perm[r]                                (remap)
//   src_offs + dst_base  scatter: source row r of partition p goes to dst_base[p] + (r - src_offs[p])      (merge, one source)
//   neither              row r -> row r, possibly between different strides                                 (export of padded rows)
//   all three            gather and scatter at once: row perm[r] goes where grouped row r belongs           (split / join)
// A row is row_bytes bytes, moved as row_bytes / width pieces of `width` bytes (16, 8, 4 or 1): the host picks the widest that
// divides both strides, row_bytes and both base addresses.
struct IuCopy {
  const uint8_t *src;
  uint8_t *dst;
  int64_t n_rows, src_stride, dst_stride;
  int row_bytes, width, nlist;
  const uint32_t *perm, *src_offs, *dst_base;
};

__global__ __launch_bounds__(256) void iu_copy_rows_kernel(IuCopy a) {
  const int cpr = a.row_bytes / a.width;
  const int64_t total = a.n_rows * cpr;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
    const int64_t r = g / cpr;
    const int c = (int)(g - r * cpr);
    int64_t sr = r, dr = r;
    if (a.perm) sr = (int64_t)a.perm[r];
    if (a.src_offs) {
      const uint32_t p = iu_partition_of(a.src_offs, a.nlist, (uint32_t)r);
      dr = (int64_t)a.dst_base[p] + (r - (int64_t)a.src_offs[p]);
    }
    const uint8_t *s = a.src + sr * a.src_stride + (int64_t)c * a.width;
    uint8_t *t = a.dst + dr * a.dst_stride + (int64_t)c * a.width;
    if (a.width == 16) *reinterpret_cast<uint4 *>(t) = *reinterpret_cast<const uint4 *>(s);
    else if (a.width == 8) *reinterpret_cast<uint64_t *>(t) = *reinterpret_cast<const uint64_t *>(s);
    else if (a.width == 4) *reinterpret_cast<uint32_t *>(t) = *reinterpret_cast<const uint32_t *>(s);
    else *t = *s;
  }
}

// flag |= 1 when two models differ in any bit (every writer stores the same word)
__global__ __launch_bounds__(256) void iu_words_differ_kernel(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, int64_t n,
                                                              uint32_t *__restrict__ flag) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    if (a[i] != b[i]) *flag = 1u;
}

// flag |= 1 unless old_ids is strictly ascending
__global__ __launch_bounds__(256) void iu_check_ascending_kernel(const uint64_t *__restrict__ old_ids, int64_t n_map, uint32_t *__restrict__ flag) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i + 1 < n_map; i += (int64_t)gridDim.x * 256)
    if (old_ids[i] >= old_ids[i + 1]) *flag = 1u;
}

// The reference's remap loop, one lane per stored row: the row's id is looked up among the OLD ids (all rows at once, so a mapping
// that swaps two ids swaps them); mapped -> new id, mapped to IU_DELETED -> the row gets no group, absent -> unchanged.
// keys[r] = the row's partition or IU_NONE (the key stable_group compacts by), ids_out[r] = its id afterwards.
__global__ __launch_bounds__(256) void iu_remap_keys_kernel(const uint64_t *__restrict__ row_ids, int64_t n, const uint32_t *__restrict__ offs,
                                                            int nlist, const uint64_t *__restrict__ old_ids, const uint64_t *__restrict__ new_ids,
                                                            int64_t n_map, uint32_t *__restrict__ keys, uint64_t *__restrict__ ids_out) {
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) {
    const uint64_t id = row_ids[r];
    int64_t lo = 0, hi = n_map;          // first position with old_ids[pos] >= id
    while (lo < hi) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if (old_ids[mid] < id) lo = mid + 1; else hi = mid;
    }
    uint64_t nid = id;
    bool dropped = false;
    if (lo < n_map && old_ids[lo] == id) {
      nid = new_ids[lo];
      dropped = nid == IU_DELETED;
    }
    keys[r] = dropped ? IU_NONE : iu_partition_of(offs, nlist, (uint32_t)r);
    ids_out[r] = nid;
  }
}
// ---- host side

static unsigned iu_grid(uint64_t items) { return grid_stride_blocks(items, 256, 65536); }

// widest piece (16 / 8 / 4 / 1 bytes) that both strides, the row length and both base addresses allow
static int iu_width(const void *src, const void *dst, int64_t src_stride, int64_t dst_stride, int row_bytes) {
  const uint64_t bits = (uint64_t)reinterpret_cast<uintptr_t>(src) | (uint64_t)reinterpret_cast<uintptr_t>(dst) | (uint64_t)src_stride |
                        (uint64_t)dst_stride | (uint64_t)row_bytes;
  if ((bits & 15) == 0) return 16;
  if ((bits & 7) == 0) return 8;
  if ((bits & 3) == 0) return 4;
  return 1;
}

int iu_copy(lance_hip_ctx *ctx, const void *src, void *dst, uint64_t n_rows, int64_t src_stride, int64_t dst_stride, int row_bytes,
            const uint32_t *perm, const uint32_t *src_offs, const uint32_t *dst_base, uint32_t nlist) {
  if (n_rows == 0 || row_bytes == 0) return LANCE_HIP_OK;
  IuCopy a;
  a.src = static_cast<const uint8_t *>(src); a.dst = static_cast<uint8_t *>(dst);
  a.n_rows = (int64_t)n_rows; a.src_stride = src_stride; a.dst_stride = dst_stride;
  a.row_bytes = row_bytes; a.width = iu_width(src, dst, src_stride, dst_stride, row_bytes); a.nlist = (int)nlist;
  a.perm = perm; a.src_offs = src_offs; a.dst_base = dst_base;
  ScopedTimer t(ctx, "index_update_copy");
  hipLaunchKernelGGL(iu_copy_rows_kernel, dim3(iu_grid(n_rows * (uint64_t)(row_bytes / a.width))), dim3(256), 0, ctx->stream, a);
  LH_CHECK_HIP(hipGetLastError());
  return LANCE_HIP_OK;
}

int iu_kind(const lance_hip_index *ix) { return ix->sq ? IU_SQ : (ix->m == 0 ? IU_FLAT : IU_PQ); }
static const char *iu_kind_name(int k) { return k == IU_SQ ? "IVF_SQ" : (k == IU_FLAT ? "IVF_FLAT" : "IVF_PQ"); }
uint32_t iu_lists(const lance_hip_index *ix) { return ix->sq ? ix->sq_nlist : ix->nlist; }
// the per-row payload next to the row ids: SQ codes (padded rows), IVF_FLAT vectors, PQ codes
uint32_t iu_stride(const lance_hip_index *ix) { return ix->sq ? ix->sq_ld : (ix->m == 0 ? ix->d * 4u : ix->code_bytes()); }
const uint8_t *iu_payload(const lance_hip_index *ix) {
  return iu_kind(ix) == IU_FLAT ? reinterpret_cast<const uint8_t *>(ix->vectors) : ix->codes;
}
uint8_t *iu_payload(lance_hip_index *ix) { return iu_kind(ix) == IU_FLAT ? reinterpret_cast<uint8_t *>(ix->vectors) : ix->codes; }

int iu_check_handle(const lance_hip_ctx *ctx, const lance_hip_index *ix, const char *what) {
  LH_REQUIRE(ix, "%s: NULL index", what);
  LH_REQUIRE(!ix->rq, "%s: IVF_RQ indices are not maintained (the reference's RabitQ storage has no append_batch): rebuild the index", what);
  LH_REQUIRE(!ix->ephemeral && ix->part_offsets && ix->part_offsets_h.size() == (size_t)iu_lists(ix) + 1 && ix->centroids,
             "%s: the handle holds no index storage", what);
  LH_REQUIRE(ix->device == ctx->device, "%s: context and index live on different devices", what);
  LH_REQUIRE(ix->n == 0 || (iu_payload(ix) && ix->row_ids), "%s: the handle holds no rows", what);
  return LANCE_HIP_OK;
}

int iu_malloc(void **out, size_t bytes) {
  const hipError_t e = hipMalloc(out, std::max<size_t>(bytes, 16));
  if (e != hipSuccess) {
    set_error("hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    return LANCE_HIP_ENOMEM;
  }
  return LANCE_HIP_OK;
}

// An empty handle with src's parameters and model (copied from src's f32 copies, never re-widened), no rows yet.  The lazy search
// constants (pt / ms / cq / raw_u8) start empty, `raw` is not inherited.  centroids / lists: another centroid array (f32, device) for
// the handle of a split / joined index (rebalance.hip); NULL: src's own.
int iu_new_like(lance_hip_ctx *ctx, const lance_hip_index *src, const float *centroids, uint32_t lists, lance_hip_index **out) {
  if (!centroids) { centroids = src->centroids; lists = iu_lists(src); }
  if (iu_kind(src) == IU_PQ) return index_alloc_like_pq_centroids(ctx, src, centroids, lists, out);      // (runs qscan_index_constants for 8-bit codes)
  auto *ix = new lance_hip_index();
  ix->device = ctx->device; ix->metric = src->metric; ix->dtype = src->dtype; ix->d = src->d; ix->m = 0; ix->nbits = src->nbits;
  ix->nlist = src->sq ? 0 : lists;        // 0 for IVF_SQ (index.h)
  ix->sq = src->sq; ix->sq_lo = src->sq_lo; ix->sq_hi = src->sq_hi; ix->sq_nlist = src->sq ? lists : 0; ix->sq_ld = src->sq_ld;
  int r = iu_malloc(reinterpret_cast<void **>(&ix->centroids), (size_t)lists * src->d * 4);
  if (r == LANCE_HIP_OK) r = iu_malloc(reinterpret_cast<void **>(&ix->part_offsets), (size_t)(lists + 1) * 4);
  if (r == LANCE_HIP_OK && hipMemcpyAsync(ix->centroids, centroids, (size_t)lists * src->d * 4, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess) {
    set_error("index update: copying the centroids failed");
    r = LANCE_HIP_ERUNTIME;
  }
  if (r != LANCE_HIP_OK) { delete ix; return r; }
  *out = ix;
  return LANCE_HIP_OK;
}

// the per-row arrays of a handle that will hold n rows
int iu_alloc_rows(lance_hip_index *ix, uint64_t n) {
  ix->n = n;
  const int kind = iu_kind(ix);
  if (kind == IU_FLAT) {
    LH_TRY(iu_malloc(reinterpret_cast<void **>(&ix->vectors), (size_t)n * ix->d * 4));
  } else if (kind == IU_SQ) {
    const size_t code_bytes = (size_t)n * ix->sq_ld;      // a multiple of 16: the sums that follow stay aligned
    LH_TRY(iu_malloc(reinterpret_cast<void **>(&ix->codes), code_bytes + (size_t)n * 4));
    ix->sq_xx = reinterpret_cast<const uint32_t *>(ix->codes + code_bytes);
  } else {
    LH_TRY(iu_malloc(reinterpret_cast<void **>(&ix->codes), (size_t)n * ix->code_bytes()));
  }
  return iu_malloc(reinterpret_cast<void **>(&ix->row_ids), (size_t)n * 8);
}

// what depends on the layout: offsets on both sides, the largest partition, IVF_FLAT's 256-row block list
int iu_finish_layout(lance_hip_ctx *ctx, lance_hip_index *ix, const lance_hip_index *src, const std::vector<uint32_t> &offs) {
  const uint32_t lists = iu_lists(ix);
  ix->part_offsets_h = offs;
  ix->model_finite = src->model_finite;      // the same model bit for bit
  ix->max_part = 0;
  for (uint32_t p = 0; p < lists; ++p) ix->max_part = std::max(ix->max_part, offs[p + 1] - offs[p]);
  LH_CHECK_HIP(hipMemcpyAsync(ix->part_offsets, ix->part_offsets_h.data(), (size_t)(lists + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
  if (iu_kind(ix) == IU_FLAT) {
    std::vector<int2_host> items;
    for (uint32_t p = 0; p < lists; ++p)
      for (uint32_t r0 = offs[p]; r0 < offs[p + 1]; r0 += 256) items.push_back(int2_host{(int)p, (int)r0});
    ix->n_flat_items = (uint32_t)items.size();
    LH_TRY(iu_malloc(reinterpret_cast<void **>(&ix->flat_items), items.size() * sizeof(int2_host)));
    if (!items.empty()) LH_CHECK_HIP(hipMemcpy(ix->flat_items, items.data(), items.size() * sizeof(int2_host), hipMemcpyHostToDevice));
  }
  LH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  return LANCE_HIP_OK;
}

// first field two sources disagree on, or NULL; models are compared afterwards, on the device
static const char *iu_first_mismatch(const lance_hip_index *a, const lance_hip_index *b) {
  if (iu_kind(a) != iu_kind(b)) return "kind";
  if (a->metric != b->metric) return "metric";
  if (a->dtype != b->dtype) return "dtype";
  if (a->d != b->d) return "d";
  if (iu_lists(a) != iu_lists(b)) return "nlist";
  if (a->m != b->m) return "m";
  if (iu_kind(a) == IU_PQ && a->nbits != b->nbits) return "nbits";
  if (a->sq && (memcmp(&a->sq_lo, &b->sq_lo, 8) != 0 || memcmp(&a->sq_hi, &b->sq_hi, 8) != 0)) return "bounds";
  return nullptr;
}

static int iu_merge(lance_hip_ctx *ctx, const lance_hip_index *const *srcs, uint32_t n_srcs, lance_hip_index *ix) {
  const lance_hip_index *s0 = srcs[0];
  const uint32_t lists = iu_lists(s0), stride = iu_stride(s0);
  // new offsets, and for every source the first destination row of each of its partitions
  std::vector<uint32_t> offs(lists + 1, 0), base((size_t)n_srcs * lists);
  for (uint32_t p = 0; p < lists; ++p) {
    uint32_t at = offs[p];
    for (uint32_t s = 0; s < n_srcs; ++s) {
      base[(size_t)s * lists + p] = at;
      at += srcs[s]->part_offsets_h[p + 1] - srcs[s]->part_offsets_h[p];
    }
    offs[p + 1] = at;
  }
  LH_TRY(iu_alloc_rows(ix, offs[lists]));
  uint32_t *base_d = ctx->scratch_t<uint32_t>("index_update.base", base.size());
  if (!base_d) return LANCE_HIP_ENOMEM;
  LH_CHECK_HIP(hipMemcpyAsync(base_d, base.data(), base.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  for (uint32_t s = 0; s < n_srcs; ++s) {
    const lance_hip_index *src = srcs[s];
    const uint32_t *b = base_d + (size_t)s * lists;
    LH_TRY(iu_copy(ctx, iu_payload(src), iu_payload(ix), src->n, stride, stride, (int)stride, nullptr, src->part_offsets, b, lists));
    LH_TRY(iu_copy(ctx, src->row_ids, ix->row_ids, src->n, 8, 8, 8, nullptr, src->part_offsets, b, lists));
    if (ix->sq) LH_TRY(iu_copy(ctx, src->sq_xx, const_cast<uint32_t *>(ix->sq_xx), src->n, 4, 4, 4, nullptr, src->part_offsets, b, lists));
  }
  return iu_finish_layout(ctx, ix, s0, offs);      // (synchronises: `base` is read by the copy above until then)
}

static int iu_remap(lance_hip_ctx *ctx, const lance_hip_index *src, const uint64_t *old_ids, const uint64_t *new_ids, uint64_t n_map,
                    lance_hip_index *ix) {
  const uint32_t lists = iu_lists(src), stride = iu_stride(src);
  const uint64_t n = src->n;
  uint32_t *keys = ctx->scratch_t<uint32_t>("index_update.keys", (size_t)(n ? n : 1));
  uint64_t *ids = ctx->scratch_t<uint64_t>("index_update.ids", (size_t)(n ? n : 1));
  uint32_t *perm = ctx->scratch_t<uint32_t>("index.perm", (size_t)(n ? n : 1));
  if (!keys || !ids || !perm) return LANCE_HIP_ENOMEM;
  if (n > 0) {
    ScopedTimer t(ctx, "index_update_keys");
    hipLaunchKernelGGL(iu_remap_keys_kernel, dim3(iu_grid(n)), dim3(256), 0, ctx->stream, src->row_ids, (int64_t)n, src->part_offsets, (int)lists,
                       old_ids, new_ids, (int64_t)n_map, keys, ids);
    LH_CHECK_HIP(hipGetLastError());
  }
  LH_TRY(stable_group(ctx, keys, (int64_t)n, (int64_t)n, (int)lists, 1, ix->part_offsets, perm, (int64_t)n, nullptr));
  std::vector<uint32_t> offs(lists + 1);
  LH_CHECK_HIP(hipMemcpyAsync(offs.data(), ix->part_offsets, (size_t)(lists + 1) * 4, hipMemcpyDeviceToHost, ctx->stream));
  LH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  LH_REQUIRE(offs[0] == 0 && offs[lists] <= n, "index_remap: grouping produced inconsistent offsets");
  LH_TRY(iu_alloc_rows(ix, offs[lists]));
  LH_TRY(iu_copy(ctx, iu_payload(src), iu_payload(ix), ix->n, stride, stride, (int)stride, perm, nullptr, nullptr, lists));
  LH_TRY(iu_copy(ctx, ids, ix->row_ids, ix->n, 8, 8, 8, perm, nullptr, nullptr, lists));
  if (ix->sq) LH_TRY(iu_copy(ctx, src->sq_xx, const_cast<uint32_t *>(ix->sq_xx), ix->n, 4, 4, 4, perm, nullptr, nullptr, lists));
  return iu_finish_layout(ctx, ix, src, offs);
}

}  // namespace lh

using namespace lh;

extern "C" int lance_hip_index_merge(lance_hip_ctx *ctx, const lance_hip_index *const *srcs, uint32_t n_srcs, lance_hip_index **out) {
  lh::CtxLock _ctx_lock(ctx);
  LH_REQUIRE(ctx && srcs && out, "index_merge: NULL argument");
  LH_REQUIRE(n_srcs >= 1 && n_srcs <= 64, "index_merge: n_srcs=%u not supported (1..64)", n_srcs);
  uint64_t total = 0;
  for (uint32_t s = 0; s < n_srcs; ++s) {
    LH_TRY(iu_check_handle(ctx, srcs[s], "index_merge"));
    const char *field = iu_first_mismatch(srcs[0], srcs[s]);
    LH_REQUIRE(!field, "index_merge: source %u (%s) differs from source 0 (%s) in %s", s, iu_kind_name(iu_kind(srcs[s])),
               iu_kind_name(iu_kind(srcs[0])), field);
    total += srcs[s]->n;
  }
  LH_REQUIRE(total < (1ull << 32), "index_merge: %llu rows in all: row offsets are 32-bit in this version", (unsigned long long)total);
  LH_CHECK_HIP(hipSetDevice(ctx->device));
  const lance_hip_index *s0 = srcs[0];
  if (n_srcs > 1) {      // the models, bit for bit, on the device: [0] centroids, [1] codebook
    uint32_t *flags = ctx->scratch_t<uint32_t>("index_update.flags", 4);
    if (!flags) return LANCE_HIP_ENOMEM;
    LH_CHECK_HIP(lh::memset_async(flags, 0, 16, ctx->stream));
    const int64_t nc = (int64_t)iu_lists(s0) * s0->d;
    const int64_t ncb = iu_kind(s0) == IU_PQ ? (int64_t)s0->m * ((int64_t)1 << s0->nbits) * (s0->d / s0->m) : 0;
    for (uint32_t s = 1; s < n_srcs; ++s) {
      if (srcs[s] == s0) continue;
      hipLaunchKernelGGL(iu_words_differ_kernel, dim3(iu_grid((uint64_t)nc)), dim3(256), 0, ctx->stream,
                         reinterpret_cast<const uint32_t *>(s0->centroids), reinterpret_cast<const uint32_t *>(srcs[s]->centroids), nc, flags);
      if (ncb > 0)
        hipLaunchKernelGGL(iu_words_differ_kernel, dim3(iu_grid((uint64_t)ncb)), dim3(256), 0, ctx->stream,
                           reinterpret_cast<const uint32_t *>(s0->codebook), reinterpret_cast<const uint32_t *>(srcs[s]->codebook), ncb, flags + 1);
    }
    LH_CHECK_HIP(hipGetLastError());
    uint32_t fh[2] = {0, 0};
    LH_CHECK_HIP(hipMemcpyAsync(fh, flags, 8, hipMemcpyDeviceToHost, ctx->stream));
    LH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    LH_REQUIRE(fh[0] == 0, "index_merge: the sources' centroids differ (every source must carry the same IVF model, bit for bit)");
    LH_REQUIRE(fh[1] == 0, "index_merge: the sources' codebook differs (every source must carry the same PQ codebook, bit for bit)");
  }
  lance_hip_index *ix = nullptr;
  LH_TRY(iu_new_like(ctx, s0, nullptr, 0, &ix));
  const int r = iu_merge(ctx, srcs, n_srcs, ix);
  if (r != LANCE_HIP_OK) { delete ix; return r; }
  *out = ix;
  return LANCE_HIP_OK;
}

extern "C" int lance_hip_index_remap(lance_hip_ctx *ctx, const lance_hip_index *src, const uint64_t *old_ids, const uint64_t *new_ids,
                                     uint64_t n_map, lance_hip_index **out) {
  lh::CtxLock _ctx_lock(ctx);
  LH_REQUIRE(ctx && out, "index_remap: NULL argument");
  LH_TRY(iu_check_handle(ctx, src, "index_remap"));
  LH_REQUIRE(n_map == 0 || (old_ids && new_ids), "index_remap: NULL mapping");
  LH_REQUIRE(n_map < (1ull << 62), "index_remap: n_map too large");
  LH_CHECK_HIP(hipSetDevice(ctx->device));
  if (n_map > 1) {
    uint32_t *flags = ctx->scratch_t<uint32_t>("index_update.flags", 4);
    if (!flags) return LANCE_HIP_ENOMEM;
    LH_CHECK_HIP(lh::memset_async(flags, 0, 16, ctx->stream));
    hipLaunchKernelGGL(iu_check_ascending_kernel, dim3(iu_grid(n_map)), dim3(256), 0, ctx->stream, old_ids, (int64_t)n_map, flags);
    LH_CHECK_HIP(hipGetLastError());
    uint32_t fh = 0;
    LH_CHECK_HIP(hipMemcpyAsync(&fh, flags, 4, hipMemcpyDeviceToHost, ctx->stream));
    LH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    LH_REQUIRE(fh == 0, "index_remap: old_ids must be strictly ascending (unsorted or duplicate ids)");
  }
  lance_hip_index *ix = nullptr;
  LH_TRY(iu_new_like(ctx, src, nullptr, 0, &ix));
  const int r = iu_remap(ctx, src, old_ids, new_ids, n_map, ix);
  if (r != LANCE_HIP_OK) { delete ix; return r; }
  *out = ix;
  return LANCE_HIP_OK;
}

extern "C" int lance_hip_index_export_rows(lance_hip_ctx *ctx, const lance_hip_index *idx, uint32_t *part_offsets_host, void *rows_host,
                                           uint32_t *aux_host, uint64_t *row_ids_host) {
  lh::CtxLock _ctx_lock(ctx);
  LH_REQUIRE(ctx, "index_export_rows: NULL argument");
  LH_TRY(iu_check_handle(ctx, idx, "index_export_rows"));
  LH_CHECK_HIP(hipSetDevice(ctx->device));
  const uint32_t lists = iu_lists(idx);
  if (part_offsets_host) memcpy(part_offsets_host, idx->part_offsets_h.data(), (size_t)(lists + 1) * 4);
  if (idx->n > 0) {
    if (rows_host && idx->sq && idx->sq_ld != idx->d) {      // padded rows: unpad on the device, one copy out
      uint8_t *tmp = ctx->scratch_t<uint8_t>("index.export", (size_t)idx->n * idx->d);
      if (!tmp) return LANCE_HIP_ENOMEM;
      LH_TRY(iu_copy(ctx, idx->codes, tmp, idx->n, idx->sq_ld, idx->d, (int)idx->d, nullptr, nullptr, nullptr, lists));
      LH_CHECK_HIP(hipMemcpyAsync(rows_host, tmp, (size_t)idx->n * idx->d, hipMemcpyDeviceToHost, ctx->stream));
    } else if (rows_host) {
      LH_CHECK_HIP(hipMemcpyAsync(rows_host, iu_payload(idx), (size_t)idx->n * iu_stride(idx), hipMemcpyDeviceToHost, ctx->stream));
    }
    if (aux_host && idx->sq) LH_CHECK_HIP(hipMemcpyAsync(aux_host, idx->sq_xx, (size_t)idx->n * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (row_ids_host) LH_CHECK_HIP(hipMemcpyAsync(row_ids_host, idx->row_ids, (size_t)idx->n * 8, hipMemcpyDeviceToHost, ctx->stream));
  }
  LH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  return LANCE_HIP_OK;
}
