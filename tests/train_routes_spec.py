"""PQ codebook training (lance_hip_pq_train, lance_amd/csrc/kmeans.hip:1062-1107) and k-means training (lance_hip_kmeans_train_ex,
kmeans.hip:723-762) on every route the E-step of kmeans_train_batched (kmeans.hip:337) can take: which route serves a call, real-valued
fixtures, and the case list.  numpy only; imported by test_train_routes_spec.py (CPU, with the oracle) and test_zz_gpu_train_routes.py.

Every Lloyd iteration calls launch_assign (kmeans.hip:410); launch_pairwise<0> (pairwise.hip:203-246) picks the kernels:

  xf_pqtrain  xf_pqtrain_kernel + pq_mfma_fix_kernel  one workgroup column per 128-column group = 128 / sd sub-quantisers, each with its own
                                                      `active` flag                              (counters: pq_mfma_estep and xf_pqtrain)
  pq_mfma     pq_mfma_estep_kernel + pq_mfma_fix_kernel                                         (counter: pq_mfma_estep)
  xf_assign   phases 1-3 of the transform kernel, carries the k-means bias                      (counters: xf_assign and ma_sweep)
  mfma        ma_top3_kernel + ma_finalize_kernel: the route of the 32-lane dot order           (counter: ma_sweep)
  mfma_wide   ma_launch_wide, K-tiled, d > 128                                                  (no counter of its own)
  fixed       pairwise_kernel<D>, d in {4, 8, 16, 32, 64, 96, 128}; workgroups of 64 or 256, a split over the centroid tiles
              (`ksplit`) merged per batch by argmin_merge_kernel                                (counter: assign alone)
  wide        pairwise_wide_kernel, any width, also batched, also with a k-split                (counter: assign alone)

Training widens float16 and int8 rows to f32 before the first iteration (kmeans.hip:737-746, :1081), so the E-step never reads a native
column and the routes depend on the element type only through the 32-lane order of float16 dot products (kmeans.hip:409).

Every case names the property it exists for (`why`); test_train_routes_spec.py establishes each on the CPU, from the oracle alone."""
import collections
import functools

import numpy as np

f32 = np.float32
NUM_CUS = 256          # MI355X; launch_fixed / launch_wide size their grids by it (pairwise.hip:179, wide.hip:322)
ROUTES = ("xf_pqtrain", "pq_mfma", "xf_assign", "mfma", "mfma_wide", "fixed", "wide")


def _cdiv(a, b):
    return -(-a // b)


# ---- which route serves an E-step --------------------------------------------------------------------------------------------------------
def pq_layout(d, m):
    """"sliced" | "row-major": the matrix lance_hip_pq_train trains on (kmeans.hip:1092; pointers on the 16-byte grid, rows * sd < 2^31)"""
    return "sliced" if m > 1 and (d // m) % 4 == 0 else "row-major"


def operand_strides(d_sub, n, batches, sliced):
    """(ldx, x_batch_off) of the training matrix: kmeans.hip:1098 sliced, :1090-1091 row-major (k-means itself passes x_batch_off = 0,
    kmeans.hip:719, with batches = 1: ldx = d decides alone there)"""
    return (d_sub, n * d_sub) if sliced else (batches * d_sub, d_sub)


def expected_route(kind, metric, d_sub, k, n, batches, has_bias, sliced):
    """One of ROUTES: a transcription of the gates of launch_pairwise<0> for the calls kmeans_train_batched makes, operand pointers on the
    16-byte grid.  n is the number of rows the trainer uses (after the caps of kmeans.hip:344 and :1075); the codebook / centroid block of
    problem b is at cent + b * k * d_sub (kmeans.hip:405)."""
    d = d_sub
    ldx, boff = operand_strides(d, n, batches, sliced)
    lanes32 = kind == "float16" and metric == "dot" and d > 16                              # kmeans.hip:409, pairwise.hip:212-215
    x_aligned = ldx % 4 == 0 and boff % 4 == 0                                              # pairwise.hip:207
    cent_aligned = (k * d) % 4 == 0 and d % 4 == 0                                          # pairwise.hip:209
    if (metric == "l2" and not has_bias and not lanes32                                     # pq_mfma.hip:286
            and d in (4, 8, 16)                                                             #   :287
            and k == 256 and n >= 2048 and batches >= 1                                     #   :288
            and x_aligned and cent_aligned                                                  #   :289
            and n < 1 << 32 and n * batches * 4 <= 256 << 20):                              #   :290-293
        if (batches * d) % 128 == 0 and ldx % 4 == 0 and boff % 4 == 0:                     # pq_mfma.hip:307 -> xform_fused.hip:1186-1189
            return "xf_pqtrain"
        return "pq_mfma"
    if (batches == 1 and not lanes32                                                        # xform_fused.hip:1216
            and d % 16 == 0 and 16 <= d <= 128 and k >= 32 and 2048 <= n < 1 << 32          #   :1218
            and x_aligned and cent_aligned):                                                #   :1219
        return "xf_assign"
    if batches == 1:                                                                        # mfma_assign.hip:781
        if d > 128:                                                                         #   :782 -> mfma_wide_supported
            dp = _cdiv(d, 32) * 32
            if d <= 4096 and not lanes32 and k >= 64 and n >= 2048 and n * dp * 4 <= 16 << 30:      # mfma_assign.hip:771-775
                return "mfma_wide"
        elif d % 16 == 0 and d >= 16 and k >= 32 and n >= 2048 and x_aligned and cent_aligned:      # mfma_assign.hip:783-790
            return "mfma"
    if cent_aligned and not lanes32 and d in (4, 8, 16, 32, 64, 96, 128):                   # pairwise.hip:220-233
        return "fixed"
    return "wide"                                                                           # pairwise.hip:237-242 -> wide.hip:319-342


def fixed_launch(d, k, n, batches, num_cus=NUM_CUS):
    """(workgroup size, ksplit) of launch_fixed (pairwise.hip:176-184)"""
    ct = min(256, 8192 // d)
    ntiles = _cdiv(k, ct)
    want = 2 * num_cus
    bs = 64 if _cdiv(n, 256) * batches * ntiles < want else 256
    blocks = _cdiv(n, bs) * batches
    return bs, (min(ntiles, 8, _cdiv(want, blocks)) if blocks < want else 1)


def wide_ksplit(k, n, batches, num_cus=NUM_CUS):
    """ksplit of launch_wide (wide.hip:320-324): tiles of 32 rows x 64 centroids"""
    rblocks = _cdiv(n, 32) * batches
    return min(_cdiv(k, 64), _cdiv(2 * num_cus, rblocks)) if rblocks < 2 * num_cus else 1


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------------
def blobs(n, d, seed, ncl=40):
    """real-valued rows: Gaussian blobs, `ncl` centres of spread 4, unit noise (sharded_kmeans_spec.blobs with more centres)"""
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((ncl, d)) * 4
    return (centers[rng.integers(0, ncl, n)] + rng.standard_normal((n, d))).astype(f32)


def integer_pairs(n, cols, seed, repeat=1):
    """a block of `cols` sub-vectors, each one of the 36 pairs (a, b), 0 <= a, b < 6 (`repeat` = 2: (a, b, a, b), still 36 values)"""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 6, (n, cols, 2))
    return np.tile(p, (1, 1, repeat)).reshape(n, cols * 2 * repeat).astype(f32)


PqCase = collections.namedtuple("PqCase", "name group route kind d m nbits n max_iters sample_rate seed data why")
KmCase = collections.namedtuple("KmCase", "name route kind metric n d k bf max_iters seed dup_init conditions why")


def pq_rows_used(c):
    """rows lance_hip_pq_train trains on (kmeans.hip:1075 the sample cap, :344 the k * 512 cap)"""
    kc = 1 << c.nbits
    rows = min(c.n, c.sample_rate * kc)
    return kc * 512 if rows >= kc * 512 else rows


def pq_route(c):
    sd = c.d // c.m
    return expected_route(c.kind, "l2", sd, 1 << c.nbits, pq_rows_used(c), c.m, False, pq_layout(c.d, c.m) == "sliced")


def km_rows_used(c):
    return c.k * 512 if c.n >= c.k * 512 else c.n


def km_route(c):
    return expected_route(c.kind, c.metric, c.d, c.k, km_rows_used(c), 1, c.bf != 0, False)


@functools.lru_cache(maxsize=None)
def pq_input(name):
    """the case's rows in their element type; cached, treat as read-only"""
    c = PQ_CASES[name]
    sd = c.d // c.m
    x = blobs(c.n, c.d, c.seed)
    if c.data.startswith("pairs"):          # "pairs:all:<repeat>" | "pairs:<sub-quantiser>:<repeat>"
        _, which, rep = c.data.split(":")
        assert sd == 2 * int(rep)
        if which == "all":
            x = integer_pairs(c.n, c.m, c.seed + 1, int(rep))
        else:
            j = int(which)
            x[:, j * sd:(j + 1) * sd] = integer_pairs(c.n, 1, c.seed + 1, int(rep))
    if c.kind == "float16":
        return x.astype(np.float16)
    if c.kind == "int8":                    # eighths of the blobs: int8 rows are integers by type, 256 levels over about +-16
        return np.clip(np.rint(x * f32(8.0)), -128, 127).astype(np.int8)
    return x


@functools.lru_cache(maxsize=None)
def km_input(name):
    """(rows in their element type, init = rows of x as the model's element type); cached, treat as read-only"""
    c = KM_CASES[name]
    x = blobs(c.n, c.d, c.seed)
    if c.metric == "dot":                   # mixed signs around the origin: rows prefer different centroids under the inner product
        x = (x - x.mean(axis=0, dtype=np.float64).astype(f32)).astype(f32)
    if c.kind == "float16":
        x = x.astype(np.float16)
    elif c.kind == "int8":
        x = np.clip(np.rint(x * f32(8.0)), -128, 127).astype(np.int8)
    pick = np.random.default_rng(c.seed + 1).permutation(km_rows_used(c))[:c.k]
    init = x[pick].astype(np.float16 if c.kind == "float16" else f32)
    if c.dup_init:                          # two copies of one row: the later one is empty after the first E-step, the trainer splits
        init[c.k // 2] = init[1]
    return x, np.ascontiguousarray(init)


def pq_oracle_rows(name):
    """what the oracle is asked: the rows the trainer uses, int8 rows as the f32 conversion the library trains on"""
    c = PQ_CASES[name]
    x = pq_input(name)[:pq_rows_used(c)]
    return x.astype(f32) if c.kind == "int8" else x


def km_oracle_rows(name):
    c = KM_CASES[name]
    x, init = km_input(name)
    x = x[:km_rows_used(c)]
    return (x.astype(f32) if c.kind == "int8" else x), init


_CACHE = {}


def pq_oracle(oracle, name):
    """(codebook, iters) of the reference on the rows the trainer uses; computed once per process, treat as read-only"""
    if ("pq", name) not in _CACHE:
        c = PQ_CASES[name]
        _CACHE["pq", name] = oracle.pq_train(pq_oracle_rows(name), c.m, nbits=c.nbits, max_iters=c.max_iters, sample_rate=c.sample_rate, seed=c.seed)
    return _CACHE["pq", name]


def km_oracle(oracle, name, bf=None):
    """(centroids, loss, iters) of the reference, computed once per process; the balance factor is divided by the length of the column,
    not of the capped prefix (kmeans.hip:708 before :344)"""
    c = KM_CASES[name]
    bf = c.bf if bf is None else bf
    if ("km", name, bf) not in _CACHE:
        x, init = km_oracle_rows(name)
        _CACHE["km", name, bf] = oracle.kmeans_train(x, c.k, max_iters=c.max_iters, tol=1e-4, balance_factor=f32(bf) / f32(c.n), init=init, seed=c.seed,
                                                     metric=c.metric)[:3]
    return _CACHE["km", name, bf]


def model_bits(a):
    """a model as unsigned words: u16 for binary16, u32 for f32"""
    a = np.ascontiguousarray(a)
    assert a.dtype in (np.float16, np.float32), a.dtype
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


# ---- the case tables ---------------------------------------------------------------------------------------------------------------------
MIXED_SEED = 1    # the blobs' and the trainer's seed of the mixed-convergence case: its first group holds iteration counts 8 and 15
BF = 1e6          # balance_factor: bf / n is far above `adjusted` in every iteration, so the adjusted factor is the one the bias is made of
BINDS = ("binds", "splits", "differs_from_bf0")


def pq_route_name(d, m):
    return expected_route("float32", "l2", d // m, 256, 3000, m, False, pq_layout(d, m) == "sliced")


def _pq_cases():
    out = collections.OrderedDict()

    def add(group, route, d, m, why, kind="float32", nbits=8, n=3000, max_iters=10, sample_rate=256, seed=None, data="blobs", name=None):
        name = name or f"{group}:{kind}:d{d}:m{m}:b{nbits}:n{n}:it{max_iters}"
        assert name not in out, name
        out[name] = PqCase(name, group, route, kind, d, m, nbits, n, max_iters, sample_rate, 1000 + len(out) if seed is None else seed, data, why)

    # width sweep, 8 bits, f32
    for d, m in ((16, 16), (16, 8), (24, 8), (48, 8), (48, 4), (40, 2)):
        sd = d // m
        add("width", "wide", d, m, f"sd {sd}: the batched wide kernel on the {pq_layout(d, m)} matrix" + (", operands off the 16-byte grid" if sd % 4 else "")
            + (f", k-split {wide_ksplit(256, 3000, m)}" if wide_ksplit(256, 3000, m) > 1 else ""))
    for d, m in ((128, 4), (128, 2), (192, 2), (256, 2)):
        sd = d // m
        add("width", "fixed", d, m, "sd %d: the batched fixed kernel on the sliced matrix, workgroups of %d, k-split %d" % ((sd,) + fixed_launch(sd, 256, 3000, m)))
    for d, m in ((64, 16), (64, 8), (96, 6)):
        add("width", "pq_mfma", d, m, f"sd {d // m}: pq_mfma_estep_kernel, batches * sd = {d} is no multiple of 128")
    for d, m in ((128, 32), (128, 16), (256, 16)):
        add("width", "xf_pqtrain", d, m, f"sd {d // m}: xf_pqtrain_kernel, {d // 128} 128-column group(s)")
    # below the matrix-core gate: sd 4 / 8 / 16 have one centroid tile at k = 256 (CT = 256), so launch_fixed takes workgroups of 64 and no
    # k-split; the k-split of the fixed kernel is on the sd 64 / 96 / 128 cases above
    for d, m in ((32, 8), (64, 8), (64, 4)):
        for n in (600, 2047, 2048):
            sd = d // m
            add("gate", "fixed" if n < 2048 else "pq_mfma", d, m,
                f"sd {sd}, n = {n}: " + ("fixed, workgroups of %d, k-split %d" % fixed_launch(sd, 256, n, m) if n < 2048 else "the first n pq_mfma takes"), n=n)
    # 4 bits
    for d, m in ((24, 8), (32, 8), (48, 4), (64, 4), (128, 4)):
        sd = d // m
        add("4bit", "wide" if sd % 4 or sd == 12 else "fixed", d, m, f"k = 16, sd {sd}: no matrix-core route below k = 256", nbits=4)
    # m = 1: row-major by the layout gate, batches = 1
    for d, route in ((16, "pq_mfma"), (64, "xf_assign"), (20, "wide"), (256, "mfma_wide")):
        add("m1", route, d, 1, f"one sub-quantiser of width {d}: {route}")
    # element types
    for d, m in ((24, 8), (64, 8), (128, 4)):
        add("types", pq_route_name(d, m), d, m, f"float16 residuals, sd {d // m}: f16 M-step, binary16 codebook", kind="float16")
    for d, m in ((24, 8), (64, 8)):
        add("types", pq_route_name(d, m), d, m, f"int8 rows, sd {d // m}: trained on the f32 conversion, f32 codebook", kind="int8")
    # sub-quantisers of one 128-column group converge on both sides of the host's convergence read at iteration 8 (kmeans.hip:400)
    add("mixed", "xf_pqtrain", 256, 16, "one group holds a sub-quantiser that stops by iteration 8 and one that stops later", max_iters=24, seed=MIXED_SEED,
        name="mixed:d256:m16")
    # empty clusters in every iteration: 36 distinct sub-vectors against 256 codewords
    add("split", "wide", 16, 8, "every sub-quantiser's block holds 36 distinct integer pairs: one RNG stream and one centroid block per sub-quantiser",
        data="pairs:all:1", max_iters=6, name="split:all:sd2")
    add("split", "wide", 16, 8, "only sub-quantiser 5 holds the integer pairs: its neighbours must not see its splits", data="pairs:5:1", max_iters=6, name="split:one:sd2")
    add("split", "pq_mfma", 32, 8, "(a, b, a, b): the same on pq_mfma, whose surrogate meets copies of one codeword", data="pairs:all:2", max_iters=6, name="split:all:sd4")
    add("split", "xf_pqtrain", 128, 8, "the pair eight times over in sub-quantiser 5 of an xf_pqtrain group", data="pairs:5:8", max_iters=6, seed=300, name="split:one:sd16")
    # caps
    add("cap", "fixed", 32, 8, "sample_rate 64 at 4 bits: the first 1024 of 3000 rows are used", nbits=4, sample_rate=64, name="cap:sample_rate")
    # iteration budget around the block of 8 iterations the host enqueues between two reads of the flags
    for it in (1, 7, 8, 9):
        add("budget", "pq_mfma", 64, 8, f"max_iters = {it}", max_iters=it, seed=77)
    return out


def _km_cases():
    out = collections.OrderedDict()

    def add(route, n, d, k, why, kind="float32", metric="l2", bf=BF, max_iters=8, seed=None, dup_init=False, conditions=BINDS, name=None):
        name = name or f"{kind}:{metric}:n{n}:d{d}:k{k}"
        assert name not in out, name
        out[name] = KmCase(name, route, kind, metric, n, d, k, bf, max_iters, 2000 + len(out) if seed is None else seed, dup_init, conditions, why)

    # (dup_init: blobs at these shapes lose no cluster by themselves; a duplicated init row empties one in the first iteration)
    add("xf_assign", 4096, 64, 48, "a bias that decides assignments on xf_assign", dup_init=True)
    add("xf_assign", 4096, 64, 48, "the same under dot", metric="dot")
    add("xf_assign", 4096, 128, 256, "d = 128, k = 256: the widest xf_assign, four centroid tiles", dup_init=True)
    add("mfma_wide", 3000, 256, 64, "the K-tiled sweep with a bias")
    add("wide", 3000, 20, 40, "the wide kernel with a bias")
    add("fixed", 4096, 32, 16, "the fixed kernel with a bias (k < 32)", dup_init=True)
    # one centroid tile (k = 48 <= CT = 128 at d = 64): workgroups of 64 and no k-split; the three cases after it split over the centroids
    add("fixed", 1500, 64, 48, "below 2048 rows: the fixed kernel, workgroups of %d, k-split %d" % fixed_launch(64, 48, 1500, 1))
    add("fixed", 1500, 64, 160, "the fixed kernel's k-split (%d): argmin_merge_kernel compares BIASED values" % fixed_launch(64, 160, 1500, 1)[1], seed=6)
    add("fixed", 1500, 128, 100, "the same at d = 128 (CT = 64), k-split %d" % fixed_launch(128, 100, 1500, 1)[1], seed=5)
    add("wide", 1500, 20, 160, "the wide kernel's k-split (%d): argmin_merge_kernel compares BIASED values" % wide_ksplit(160, 1500, 1))
    add("wide", 6000, 32, 24, "float16 under dot: 32-lane order, the two-pass wide kernel, f16 M-step", kind="float16", metric="dot", conditions=("differs_from_bf0",))
    add("mfma", 4096, 64, 48, "float16 under dot at k >= 32: the 32-lane order on ma_top3_kernel, with a bias", kind="float16", metric="dot",
        conditions=("differs_from_bf0",))
    add("fixed", 6000, 32, 24, "int8 rows: trained on the f32 conversion, f32 centroids", kind="int8", conditions=("differs_from_bf0",))
    add("xf_assign", 4096, 64, 48, "int8 rows on xf_assign", kind="int8", conditions=("differs_from_bf0",))
    add("fixed", 3000, 16, 4, "n >= k * 512: the first 2048 of 3000 rows are used, the balance factor is still divided by 3000", bf=1.0, conditions=(),
        name="cap:k512")
    return out


PQ_CASES = _pq_cases()
KM_CASES = _km_cases()
PQ_GROUPS = tuple(collections.OrderedDict((c.group, 1) for c in PQ_CASES.values()))


def pq_group(group):
    return [c for c in PQ_CASES.values() if c.group == group]
