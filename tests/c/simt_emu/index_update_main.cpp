// index_update_main.cpp -- the device code of lance_amd/csrc/index_update.hip on the CPU, a thread per lane (simt_emu.h), built with
// AddressSanitizer + UBSan by tests/test_index_update_kernels_cpu.py, which cuts the kernels' text (and the host's choice of the
// access width) out of the source into index_update_device_code.inc.  Every buffer is a heap block of exactly the bytes the engine
// would allocate, so an index that strays by one element is reported.  stable_group (group.hip, wave intrinsics) is replaced by a
// host stable sort: only the new kernels are emulated.
//
//   in : u32 mode (0 merge, 1 remap), nlist, stride, misalign (bytes added to every payload base), has_aux, unpad (row bytes of an
//        extra unpadding copy of the result, 0 = none), n_srcs;  per source: u32 n, offs[nlist + 1], payload[n * stride], u64 ids[n],
//        u32 aux[n] (if has_aux);  remap: u32 n_map, u64 old[n_map], u64 new[n_map]
//   out: u32 refused, n_out, offs[nlist + 1], payload[n_out * stride], u64 ids[n_out], u32 aux[n_out] (if has_aux),
//        unpadded payload[n_out * unpad] (if unpad)
#include "simt_emu.h"

#include <numeric>

#include "index_update_device_code.inc"

struct Block {      // exactly `bytes` usable bytes starting `shift` bytes into a malloc block that ends with them
  uint8_t *base = nullptr, *p = nullptr;
  size_t bytes = 0;
  Block() = default;
  Block(size_t n, size_t shift) : base(static_cast<uint8_t *>(malloc(n + shift + (n + shift == 0)))), p(base + shift), bytes(n) {}
  Block(const Block &) = delete;
  Block(Block &&o) : base(o.base), p(o.p), bytes(o.bytes) { o.base = nullptr; }
  Block &operator=(Block &&o) {
    if (this != &o) { free(base); base = o.base; p = o.p; bytes = o.bytes; o.base = nullptr; }
    return *this;
  }
  ~Block() { free(base); }
};

struct Source {
  uint32_t n = 0;
  std::vector<uint32_t> offs;
  Block payload, ids, aux, offs_d;
};

static FILE *fin, *fout;
static void rd(void *p, size_t bytes) { if (bytes && fread(p, 1, bytes, fin) != bytes) { fprintf(stderr, "short input\n"); exit(2); } }
static void wr(const void *p, size_t bytes) { if (bytes && fwrite(p, 1, bytes, fout) != bytes) { fprintf(stderr, "short output\n"); exit(2); } }
static uint32_t rd32() { uint32_t v; rd(&v, 4); return v; }

// iu_copy of index_update.hip: the same width choice (iu_width, cut from the source), the kernel on two workgroups
static void copy_rows(const void *src, void *dst, uint64_t n_rows, int64_t src_stride, int64_t dst_stride, int row_bytes, const uint32_t *perm,
                      const uint32_t *src_offs, const uint32_t *dst_base, uint32_t nlist) {
  if (n_rows == 0 || row_bytes == 0) return;
  IuCopy a;
  a.src = static_cast<const uint8_t *>(src); a.dst = static_cast<uint8_t *>(dst);
  a.n_rows = (int64_t)n_rows; a.src_stride = src_stride; a.dst_stride = dst_stride;
  a.row_bytes = row_bytes; a.width = iu_width(src, dst, src_stride, dst_stride, row_bytes); a.nlist = (int)nlist;
  a.perm = perm; a.src_offs = src_offs; a.dst_base = dst_base;
  const uint64_t all = (uint64_t)reinterpret_cast<uintptr_t>(src) | (uint64_t)reinterpret_cast<uintptr_t>(dst) | (uint64_t)src_stride |
                       (uint64_t)dst_stride | (uint64_t)row_bytes;
  if ((a.width != 16 && a.width != 8 && a.width != 4 && a.width != 1) || all % (uint64_t)a.width != 0) {
    fprintf(stderr, "width %d does not fit the operands\n", a.width);
    exit(3);
  }
  printf("copy width %d\n", a.width);
  simt_launch(2, 1, 256, [&] { iu_copy_rows_kernel(a); });
}

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  fin = fopen(argv[1], "rb"); fout = fopen(argv[2], "wb");
  if (!fin || !fout) return 2;
  const uint32_t mode = rd32(), nlist = rd32(), stride = rd32(), shift = rd32(), has_aux = rd32(), unpad = rd32(), n_srcs = rd32();
  std::vector<Source> srcs(n_srcs);
  for (auto &s : srcs) {
    s.n = rd32();
    s.offs.resize(nlist + 1);
    rd(s.offs.data(), (nlist + 1) * 4);
    s.payload = Block((size_t)s.n * stride, shift); rd(s.payload.p, s.payload.bytes);
    s.ids = Block((size_t)s.n * 8, 0); rd(s.ids.p, s.ids.bytes);
    s.aux = Block(has_aux ? (size_t)s.n * 4 : 0, 0); rd(s.aux.p, s.aux.bytes);
    s.offs_d = Block((nlist + 1) * 4, 0); memcpy(s.offs_d.p, s.offs.data(), (nlist + 1) * 4);
  }
  uint32_t refused = 0, n_out = 0;
  std::vector<uint32_t> offs(nlist + 1, 0);
  Block payload, ids, aux;
  if (mode == 0) {      // ---- merge: the host part of iu_merge, then one copy per array and source
    std::vector<uint32_t> base((size_t)n_srcs * nlist);
    for (uint32_t p = 0; p < nlist; ++p) {
      uint32_t at = offs[p];
      for (uint32_t s = 0; s < n_srcs; ++s) { base[(size_t)s * nlist + p] = at; at += srcs[s].offs[p + 1] - srcs[s].offs[p]; }
      offs[p + 1] = at;
    }
    n_out = offs[nlist];
    payload = Block((size_t)n_out * stride, shift); ids = Block((size_t)n_out * 8, 0); aux = Block(has_aux ? (size_t)n_out * 4 : 0, 0);
    Block base_d(base.size() * 4, 0);
    memcpy(base_d.p, base.data(), base.size() * 4);
    for (uint32_t s = 0; s < n_srcs; ++s) {
      const uint32_t *so = reinterpret_cast<const uint32_t *>(srcs[s].offs_d.p), *b = reinterpret_cast<const uint32_t *>(base_d.p) + (size_t)s * nlist;
      copy_rows(srcs[s].payload.p, payload.p, srcs[s].n, stride, stride, (int)stride, nullptr, so, b, nlist);
      copy_rows(srcs[s].ids.p, ids.p, srcs[s].n, 8, 8, 8, nullptr, so, b, nlist);
      if (has_aux) copy_rows(srcs[s].aux.p, aux.p, srcs[s].n, 4, 4, 4, nullptr, so, b, nlist);
    }
  } else {              // ---- remap: ascending check, keys, (host) stable grouping, gathers
    const Source &s = srcs[0];
    const uint32_t n_map = rd32();
    Block old_ids((size_t)n_map * 8, 0), new_ids((size_t)n_map * 8, 0), flag(4, 0);
    rd(old_ids.p, old_ids.bytes); rd(new_ids.p, new_ids.bytes);
    const uint64_t *oldp = reinterpret_cast<const uint64_t *>(old_ids.p), *newp = reinterpret_cast<const uint64_t *>(new_ids.p);
    memset(flag.p, 0, 4);
    if (n_map > 1) simt_launch(2, 1, 256, [&] { iu_check_ascending_kernel(oldp, (int64_t)n_map, reinterpret_cast<uint32_t *>(flag.p)); });
    memcpy(&refused, flag.p, 4);
    if (!refused) {
      Block keys((size_t)s.n * 4, 0), ids_tmp((size_t)s.n * 8, 0), perm((size_t)s.n * 4, 0);
      uint32_t *kp = reinterpret_cast<uint32_t *>(keys.p);
      if (s.n > 0)
        simt_launch(2, 1, 256, [&] {
          iu_remap_keys_kernel(reinterpret_cast<const uint64_t *>(s.ids.p), (int64_t)s.n, reinterpret_cast<const uint32_t *>(s.offs_d.p), (int)nlist, oldp, newp,
                               (int64_t)n_map, kp, reinterpret_cast<uint64_t *>(ids_tmp.p));
        });
      // stable_group's contract: offsets per key, and the rows with a key < nlist grouped by key in ascending row order
      std::vector<uint32_t> order;
      for (uint32_t r = 0; r < s.n; ++r) {
        if (kp[r] != IU_NONE && kp[r] >= nlist) { fprintf(stderr, "key %u out of range at row %u\n", kp[r], r); return 3; }
        if (kp[r] != IU_NONE) { order.push_back(r); ++offs[kp[r] + 1]; }
      }
      std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return kp[a] < kp[b]; });
      for (uint32_t p = 0; p < nlist; ++p) offs[p + 1] += offs[p];
      n_out = offs[nlist];
      if (n_out) memcpy(perm.p, order.data(), (size_t)n_out * 4);
      const uint32_t *pp = reinterpret_cast<const uint32_t *>(perm.p);
      payload = Block((size_t)n_out * stride, shift); ids = Block((size_t)n_out * 8, 0); aux = Block(has_aux ? (size_t)n_out * 4 : 0, 0);
      copy_rows(s.payload.p, payload.p, n_out, stride, stride, (int)stride, pp, nullptr, nullptr, nlist);
      copy_rows(ids_tmp.p, ids.p, n_out, 8, 8, 8, pp, nullptr, nullptr, nlist);
      if (has_aux) copy_rows(s.aux.p, aux.p, n_out, 4, 4, 4, pp, nullptr, nullptr, nlist);
    }
  }
  wr(&refused, 4); wr(&n_out, 4); wr(offs.data(), (nlist + 1) * 4);
  wr(payload.p, payload.bytes); wr(ids.p, ids.bytes); wr(aux.p, aux.bytes);
  if (unpad) {          // lance_hip_index_export_rows of padded rows
    Block flat((size_t)n_out * unpad, 0);
    copy_rows(payload.p, flat.p, n_out, stride, unpad, (int)unpad, nullptr, nullptr, nullptr, nlist);
    wr(flat.p, flat.bytes);
  }
  fclose(fout);
  puts("ok");
  return 0;
}
