/*
 * vaexhip.h -- C-ABI of libvaexhip.so, the MI355X (gfx950) implementation of
 * vaex-core's binned-statistics and groupby-aggregation hot path.
 *
 * The boundary is plain C: opaque handles, raw pointers + sizes, int status
 * codes and a thread-local last-error string.  No torch / pybind11 types.
 * Every entry point names the reference interface it replaces
 * (paths relative to the reference root, packages/vaex-core/src unless noted).
 *
 * Pointer arguments tagged `loc` may point to host memory (VH_LOC_HOST: staged
 * to HBM by the library, pipelined per chunk) or to HBM (VH_LOC_DEVICE: read in
 * place); VH_LOC_AUTO asks the HIP runtime.  Like the reference (which stores
 * raw pointers from py::buffer without incref, superagg_binners.cpp:63-73),
 * the caller keeps column buffers alive until vh_grid_bin returns.
 */
#ifndef VAEXHIP_H
#define VAEXHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VH_ABI_VERSION 1

/* status codes; VH_ERR_RUNTIME mirrors the std::runtime_error the reference
 * throws ("Expected a 1d array", "Itemsize of data and binner are not equal",
 * "data not set", "data2 not set", "no binners set and no length given"). */
enum vh_status {
    VH_OK = 0,
    VH_ERR_RUNTIME = 1,
    VH_ERR_HIP = 2,
    VH_ERR_NOMEM = 3,
    VH_ERR_ARG = 4
};

/* dtype codes, same order as the reference's per-dtype bindings
 * (superagg_binners.cpp:279-303, superagg.cpp:614-624) */
enum vh_dtype {
    VH_F64 = 0, VH_F32 = 1, VH_I64 = 2, VH_I32 = 3, VH_I16 = 4, VH_I8 = 5,
    VH_U64 = 6, VH_U32 = 7, VH_U16 = 8, VH_U8 = 9, VH_BOOL = 10
};

enum vh_loc { VH_LOC_AUTO = 0, VH_LOC_HOST = 1, VH_LOC_DEVICE = 2 };

/* aggregator kinds (superagg.cpp:547-555) */
enum vh_agg_kind {
    VH_AGG_COUNT = 0,      /* AggCount_<t>      superagg.cpp:155-192 */
    VH_AGG_SUM = 1,        /* AggSum_<t>        superagg.cpp:349-389 */
    VH_AGG_MIN = 2,        /* AggMin_<t>        superagg.cpp:241-287 */
    VH_AGG_MAX = 3,        /* AggMax_<t>        superagg.cpp:194-239 */
    VH_AGG_FIRST = 4,      /* AggFirst_<t>      superagg.cpp:436-511 */
    VH_AGG_SUM_MOMENT = 5, /* AggSumMoment_<t>  superagg.cpp:391-434 */
    VH_AGG_NUNIQUE = 6,    /* AggNUnique_<t>    agg_hash_primitive.cpp:6-102; create arg: bit 0
                              dropmissing, bit 1 dropnan */
    VH_AGG_COV = 7         /* op_cov            vaexfast.cpp:1070-1104 (TaskStatistic OP_COV,
                              vaex/tasks.py:191-201) over the superagg binners; VH_F64 only;
                              create arg: the number of value columns N, 1..8, each set with
                              vh_agg_set_data(index < N).  The grid image (download / upload /
                              info) is float64 [cell][2N + 2N^2]: N counts, N sums, N x N pair
                              counts, N x N pair sums (entry r + c * N); uploading takes the
                              entries r <= c and the column counts for the diagonal counts.
                              vh_agg_device_ptr gives the 2N + N^2 distinct accumulators. */
};

/* reductions of the multi-GPU collectives */
enum vh_op { VH_OP_SUM = 0, VH_OP_MIN = 1, VH_OP_MAX = 2 };

typedef struct vh_binner vh_binner;
typedef struct vh_grid vh_grid;
typedef struct vh_agg vh_agg;
typedef struct vh_set vh_set;
typedef struct vh_counter vh_counter;

/* ---- library / device plumbing ---------------------------------------- */
const char *vh_last_error(void);
int vh_abi_version(void);
int vh_device_count(int *count);
int vh_set_device(int device);
int vh_get_device(int *device);
int vh_synchronize(void);
int vh_malloc(void **dptr, uint64_t bytes);
int vh_free(void *dptr);
/* page-locked host blocks (cached; result arrays are read back through them) */
int vh_host_alloc(void **ptr, uint64_t bytes);
int vh_host_free(void *ptr, uint64_t bytes);
/* Register a page-aligned host range (typically a column memory-mapped from a file) for
 * direct DMA: host columns whose chunks lie inside it stream to HBM with no bounce copy.
 * The range must stay mapped until vh_host_unregister(ptr) (which drains the device). */
/* free the page-locked blocks the library caches for read-backs and pipeline buffers
 * (capped per process: VAEX_AMD_PINNED_CACHE_MB, else 8 GiB / LOCAL_WORLD_SIZE) */
int vh_host_cache_trim(void);
/* free the device blocks the library keeps for reuse on the calling thread's device
 * (freed scratch and DeviceArray buffers, at most 1/8 of the device's memory; the dense
 * rank's sort scratch); the next query allocates afresh */
int vh_device_cache_trim(void);
int vh_host_register(void *ptr, uint64_t bytes);
int vh_host_unregister(void *ptr);
int vh_memcpy_htod(void *dst, const void *src, uint64_t bytes);
int vh_memcpy_dtoh(void *dst, const void *src, uint64_t bytes);
int vh_memcpy_dtod(void *dst, const void *src, uint64_t bytes);
int vh_memset(void *dptr, int value, uint64_t bytes);
/* synthetic columns generated in HBM (bench/test data; counter-based
 * splitmix64, so any sub-range can be regenerated on the host):
 * dist 0 = uniform [a, b), 1 = normal(mean a, sd b): F64, or F32 (the
 *      float64 draw rounded),
 *      2 = uniform integer [a, b) stored as `dtype` (I8/I32/I64),
 *      3 = sorted: a + b * normal quantile of (i + 0.5) / n (f64, ascending),
 *      4 = sorted integers [a, b) in equal consecutive runs (I32/I64). */
int vh_fill_random(void *dptr, uint64_t n, int dtype, int dist, uint64_t seed, double a, double b);
/* kernel timing with hipEvents on the library stream (bench roofline) */
int vh_timing_enable(int on);
int vh_timing_reset(void);
int vh_timing_read(const char *kernel, uint64_t *launches, double *total_ms);
int vh_stream(void **stream);
/* engine statistics since the last reset (this device): "tile_overflow_rows" (tile path rows
 * that missed their pass-A region and took global atomics), "hashagg_overflow_rows",
 * "set_overflow_rows" (the groupby / ordered_set partition overflow paths); the maximum since
 * the last reset, every device: "tile_stream_rounds" (rounds of the longest segment walk of a
 * tile path pass-B unit in the stream layout, counted on the host from the planned units);
 * host images (vh_agg_set_host_image), every device, host counts: "host_image_bins" (bins
 * that left at least one registered image current), "host_image_tile_units" (the most pass-B
 * units that shared one tile's ticket in a mirrored launch: a maximum) */
int vh_stat_read(const char *name, uint64_t *value, int reset);

/* ---- Binners: superagg_binners.cpp ------------------------------------- */
/* BinnerScalar_<dtype>[_non_native](expression, vmin, vmax, bins)
 * superagg_binners.cpp:5-93 (ctor :9, to_bins :14-56) */
int vh_binner_scalar_create(const char *expression, int dtype, int flip_endian, double vmin,
                            double vmax, uint64_t bins, vh_binner **out);
/* BinnerOrdinal_<dtype>[_non_native](expression, ordinal_count, min_value)
 * superagg_binners.cpp:95-184; both arguments already converted to uint64_t
 * the way the C++ ctor converts its T arguments (:99). */
int vh_binner_ordinal_create(const char *expression, int dtype, int flip_endian,
                             uint64_t ordinal_count, uint64_t min_value, vh_binner **out);
/* BinnerOrdinal over _ordinal_values(key, set) (functions.py:2441-2448 +
 * hash_primitives.hpp:556-583) fused into one binner: reads the raw key
 * column and probes the GPU set inside the bin kernel. */
int vh_binner_set_ordinal_create(const char *expression, vh_set *set, uint64_t ordinal_count,
                                 vh_binner **out);
int vh_binner_copy(const vh_binner *binner, vh_binner **out);   /* .copy() */
int vh_binner_destroy(vh_binner *binner);
/* set_data(buf): ndim must be 1 ("Expected a 1d array"), itemsize must match
 * ("Itemsize of data and binner are not equal"), superagg_binners.cpp:63-73 */
int vh_binner_set_data(vh_binner *binner, const void *ptr, uint64_t length, int itemsize, int ndim,
                       int loc);
int vh_binner_set_data_mask(vh_binner *binner, const uint8_t *mask, uint64_t length, int ndim,
                            int loc);                           /* :78-85, 1 = masked */
int vh_binner_clear_data_mask(vh_binner *binner);             /* :74-77 */
int vh_binner_shape(const vh_binner *binner, uint64_t *shape); /* bins+3 / count+3 */
int vh_binner_size(const vh_binner *binner, uint64_t *size);

/* ---- Grid: agg.hpp:50-143 ----------------------------------------------- */
int vh_grid_create(vh_binner *const *binners, int nbinners, vh_grid **out);
int vh_grid_destroy(vh_grid *grid);
/* shapes/strides must hold >= dims entries (agg.hpp:54-69: strides[0] = 1) */
int vh_grid_info(const vh_grid *grid, int *dims, uint64_t *shapes, uint64_t *strides,
                 uint64_t *length1d);
/* Grid.bin(aggs[, length]) agg.hpp:76-105; has_length = 0 takes the first
 * binner's size and fails with "no binners set and no length given". */
int vh_grid_bin(vh_grid *grid, vh_agg *const *aggs, int naggs, uint64_t length, int has_length);

/* ---- Aggregators: superagg.cpp ----------------------------------------- */
/* Agg<Kind>_<dtype>[_non_native](grid[, moment]) -- `arg` is the moment of
 * AggSumMoment, the flags of AggNUnique, the column count of AggCov, ignored otherwise.
 * The grid lives in HBM. */
int vh_agg_create(vh_grid *grid, int kind, int dtype, int flip_endian, uint32_t arg, vh_agg **out);
int vh_agg_destroy(vh_agg *agg);
/* set_data(buf, index): index 1 = the order column of AggFirst (:449-461) */
int vh_agg_set_data(vh_agg *agg, const void *ptr, uint64_t length, int itemsize, int ndim, int index,
                    int loc);
int vh_agg_set_data_mask(vh_agg *agg, const uint8_t *mask, uint64_t length, int ndim, int loc); /* 1 = keep */
int vh_agg_clear_data_mask(vh_agg *agg);
/* AggNUnique::set_selection_mask (agg_hash_primitive.cpp:82-89): with a selection set, rows
 * whose data mask is 0 are outside the selection (skipped), not missing values */
int vh_agg_set_selection_mask(vh_agg *agg, const uint8_t *mask, uint64_t length, int ndim, int loc);
/* AggNUnique state to / from host memory (multi-GPU combine, counter::merge
 * hash_primitives.hpp:393-415): export with null arrays returns the deduplicated pair
 * count in *n; nulls / nans hold one count per grid cell; import appends and adds */
int vh_agg_nunique_export(vh_agg *agg, uint64_t *n, uint64_t *cells, uint64_t *vals, uint64_t *nulls, uint64_t *nans);
int vh_agg_nunique_import(vh_agg *agg, uint64_t n, const uint64_t *cells, const uint64_t *vals, const uint64_t *nulls,
                          const uint64_t *nans);
/* __sizeof__ (grid bytes, agg.hpp:162-164), grid dtype and itemsize */
int vh_agg_info(const vh_agg *agg, uint64_t *bytes, int *grid_dtype, uint64_t *itemsize);
/* buffer protocol (agg.hpp:166-179): the grid is copied to/from a host image */
int vh_agg_download(vh_agg *agg, void *host, uint64_t bytes);
int vh_agg_upload(vh_agg *agg, const void *host, uint64_t bytes);
int vh_agg_download_order(vh_agg *agg, void *host, uint64_t bytes); /* AggFirst order grid */
/* (new) Registers `host` as the aggregator's host image: page-locked, mapped memory (vh_host_alloc,
 * hipHostMalloc), 16-byte aligned, bytes == length1d * itemsize and >= 256 KiB; host == NULL
 * clears the registration.  VH_ERR_ARG for anything else (pageable memory included) and for an
 * AggCov.  While an image is registered, a vh_grid_bin of count / sum / sum-moment aggregators
 * over device columns that takes the tiled engine writes every finished tile of the grid into
 * the image from inside its last kernel, and vh_agg_download(agg, host, bytes) into that same
 * image is then a stream synchronize and no copy.  Every other write of the device grid (a bin
 * on another route, vh_agg_upload, vh_agg_reduce, vh_comm_agg_allreduce) leaves the image stale
 * and the next download an ordinary copy; vh_agg_device_ptr drops the registration.  The memory must stay valid until
 * the registration is cleared, replaced or dropped, or the aggregator destroyed: each of those
 * waits for the library stream first.  VH_HOST_IMAGE=0 (read per bin) turns the mirror off. */
int vh_agg_set_host_image(vh_agg *agg, void *host, uint64_t bytes);
/* Nonzero cells of grid items [begin, end): out3 = {count, first index, last index} relative to
 * begin ({0, -1, -1} when none) -- the occupied range of a dense groupby's count(*) grid, found
 * on the device (groupby.py:484-533 keeps the cells with count > 0). */
int vh_agg_occupancy(vh_agg *agg, uint64_t begin, uint64_t end, int64_t *out3);
/* percentile finish of an AggCount grid whose last binner is the percentile axis
 * (dataframe.py:1419-1555 finish + vaexfast.cpp:1574-1628 grid_find_edges), on the device:
 * out[npct][outer central cells] float64, host memory (outer cells in Fortran order of the
 * outer axes' central parts, slots 2..shape-2).  lo, hi: the percentile axis' limits.
 * VH_ERR_ARG: not an AggCount, no binners, npct < 1, a percentage that is NaN or outside
 * [0, 100], out_items != npct * prod(outer shape - 3). */
int vh_agg_percentile(vh_agg *agg, const double *percentages, int npct, double lo, double hi,
                      double *out, uint64_t out_items);
/* mutual information finish of an AggCount grid whose binners 0 and 1 are the x and y axes and
 * whose binners 2.. are the outer (binby) axes (dataframe.py:622-718 calculate +
 * kld.py:13-21 + utils.py:119-142), on the device: out[outer central cells] float64, host
 * memory (Fortran order of the outer axes' central parts, as vh_agg_percentile).  Per cell over
 * the central Mx x My part of its x-y slab (every edge slot of every axis ignored):
 * sum over a > 0 of p * log(p / q), p = a / T, q = rx * cy / (T * T); an empty cell gives 0.
 * The float64 sum has a fixed order per shape: two calls on one grid agree bit for bit.
 * VH_ERR_ARG: not an AggCount with an int64 grid, fewer than 2 or more than 16 binners, an x or
 * y axis of shape < 4, out_items != prod(outer shape - 3), out null with cells to write. */
int vh_agg_mutual_information(vh_agg *agg, double *out, uint64_t out_items);
int vh_agg_upload_order(vh_agg *agg, const void *host, uint64_t bytes);   /* (new) combine across ranks */
int vh_agg_device_ptr(vh_agg *agg, void **grid_dptr, void **grid2_dptr);
/* Aggregator.reduce(list) superagg.cpp:160-167, 205-212, 252-259, 354-361, 470-480 */
int vh_agg_reduce(vh_agg *agg, vh_agg *const *others, int nothers);

/* ---- ordered_set_<dtype>: hash_primitives.hpp:417-621 ------------------- */
int vh_set_create(int dtype, vh_set **out);
int vh_set_destroy(vh_set *set);
/* update(keys[, mask]) hash_primitives.hpp:96-281 (mask: 1 = null) */
int vh_set_update(vh_set *set, const void *keys, const uint8_t *mask, uint64_t n, int loc);
/* update with only the rows where select[i] != 0 (a filtered / selected chunk, without
 * compacting it first; ordinals follow the first selected occurrence) */
int vh_set_update_selected(vh_set *set, const void *keys, const uint8_t *mask, const uint8_t *select, uint64_t n,
                           int loc);
/* assigns ordinals (first-appearance order); called implicitly by the readers */
int vh_set_seal(vh_set *set);
/* len(set), nan_count, null_count, nan_value, null_value (ordinals; 0x7fffffff if absent) */
int vh_set_info(vh_set *set, int64_t *length, int64_t *nan_count, int64_t *null_count,
                int64_t *nan_value, int64_t *null_value);
/* key_array() hash_primitives.hpp:289-312 -- out has `length` items of the key dtype */
int vh_set_key_array(vh_set *set, void *out_host);
/* map_ordinal(keys) hash_primitives.hpp:543-583: out_itemsize 1/2/4/8; -1 = unknown key */
int vh_set_map_ordinal(vh_set *set, const void *keys, uint64_t n, int loc, void *out, int out_itemsize,
                       int out_loc);

/* ---- counter_<dtype>: hash_primitives.hpp:328-415 (key -> occurrence count) ------------ */
/* Key identity is the ordered set's: one NaN entry, one null entry (mask byte set), every
 * other key by bit pattern.  initial_capacity: slots of the first table (a power of two
 * >= 16), 0 = the default; the table grows as needed and a chunk is never counted twice. */
int vh_counter_create(int dtype, uint64_t initial_capacity, vh_counter **out);
int vh_counter_destroy(vh_counter *counter);
/* update(keys[, mask]): every row counts 1.  mask may be NULL (1 = missing); select may be
 * NULL, rows with select[i] == 0 are not seen at all (as vh_set_update_selected) */
int vh_counter_update(vh_counter *counter, const void *keys, const uint8_t *mask, const uint8_t *select, uint64_t n,
                      int loc);
/* row i adds counts[i] (> 0; rows with 0 are skipped): counter::merge and un-pickling */
int vh_counter_add(vh_counter *counter, const void *keys, const uint8_t *mask, const int64_t *counts, uint64_t n,
                   int loc);
/* length = distinct regular keys + (nan_count > 0) + (null_count > 0) */
int vh_counter_info(vh_counter *counter, int64_t *length, int64_t *nan_count, int64_t *null_count);
/* The finish on the device.  order 0: NaN (index 0), null (next index), then the regular
 * keys ascending (-0.0 before 0.0); 1: that list stably sorted by count ascending; 2: the
 * exact reverse of 1.  dropnan / dropmissing leave the NaN / null entry out.  keys_out (key
 * dtype) and counts_out are host arrays of `length` items; n_out items are written.  The
 * null entry's key is 0 and its index is *null_index (-1 when absent). */
int vh_counter_read(vh_counter *counter, int order, int dropnan, int dropmissing, void *keys_out, int64_t *counts_out,
                    uint64_t *n_out, int64_t *null_index);

/* ---- limits pre-pass: vaexfast.cpp:1043-1055 (op_min_max) --------------- */
int vh_minmax(const void *data, uint64_t n, int dtype, int flip_endian, const uint8_t *mask, int loc,
              double *out_min, double *out_max);
/* min / max (as double, NaN ignored) of `nsample` evenly spaced rows (row j * n / nsample) of
 * a native, unmasked HBM column: the speculative key range of a dense single-key groupby
 * (vaex_amd/groupby.py _dense_range).  No reference counterpart: the reference's Grouper
 * builds an ordered_set instead (groupby.py:97-168); the caller verifies the guess with the
 * grid's under/overflow cells (superagg_binners.cpp:104-142 bins out-of-range keys there)
 * and redoes the query with the exact vh_minmax range when they are not empty. */
int vh_minmax_sample(const void *data, uint64_t n, int dtype, uint64_t nsample, double *out_min, double *out_max);

/* ---- fused hash groupby (hashagg.hip) ------------------------------------
 * groupby(key).agg({count(*), count(v), sum(v), mean(v)}) for one integer key column
 * (any width) and up to 2 value columns, in one hash-partitioned pass.  Replaces, for that
 * query shape, Grouper pass 1 (ordered_set update, hash_primitives.hpp:96-281) +
 * _ordinal_values/map_ordinal (hash_primitives.hpp:543-583) + BinnerOrdinal
 * (superagg_binners.cpp:104-142) + AggCount/AggSum (superagg.cpp:155-192,349-389), as
 * driven by groupby.py:97-168,484-533.  Groups come out sorted by key. */
typedef struct vh_hashagg vh_hashagg;
/* nonnull_mask: bit v set = the non-NaN count of value column v is read (count(v), mean);
 * the counts of other float columns are left undefined */
int vh_hashagg_create(int key_dtype, int nvals, const int *val_dtypes, uint32_t nonnull_mask, vh_hashagg **out);
int vh_hashagg_destroy(vh_hashagg *h);
/* one chunk of rows (may be called repeatedly); VH_ERR_RUNTIME on a table overflow
 * (the caller then falls back to the ordered_set path) */
int vh_hashagg_update(vh_hashagg *h, const void *keys, const void *const *vals, uint64_t n, int loc);
int vh_hashagg_finish(vh_hashagg *h, uint64_t *ngroups);
/* outputs, ngroups items each: keys as int64, count(*) int64, per value column its sum
 * (8 bytes: double for float columns, int64/uint64 for integers) and non-NaN count int64;
 * any output may be host or HBM memory (a caller that decodes combined multi-key keys on the
 * device keeps them there) */
int vh_hashagg_read(vh_hashagg *h, int64_t *keys, int64_t *counts, void *const *sums, int64_t *const *nonnull);
/* after vh_hashagg_finish: reorder the groups by the row each key first appears at -- the
 * ordinal order of an ordered_set built over the same keys (hash_primitives.hpp:96-281,289-312;
 * groupby(key, assume_sparse=True, sort=False), groupby.py:97-168) -- so vh_hashagg_read
 * returns them in that order.  `keys` is the whole key column the updates saw, in order (n =
 * their total rows).  A prefix of the rows is scanned until every group has its first row
 * (run heads only); keys that first appear late fall back to an ordered_set over all rows. */
int vh_hashagg_order_first(vh_hashagg *h, const void *keys, uint64_t n, int loc);
/* the same first-appearance order for the groups of a dense integer key range (the grid
 * route of groupby(key, assume_sparse=True)): labels[0..m) are the keys of the result groups
 * (int64, host or HBM; every one occurs in `keys`, all within [vmin, vmin + span)), and
 * perm[i] (host, int64) is the label index of the i-th group in the order the keys first
 * appear in the key column (n rows, host or HBM) -- an ordered_set's ordinal order
 * (hash_primitives.hpp:96-281).  A prefix of run heads is scanned until every label is seen. */
int vh_dense_first_order(const void *keys, uint64_t n, int loc, int key_dtype, int64_t vmin, uint64_t span,
                         const int64_t *labels, uint64_t m, int64_t *perm);
/* groupby(int key, assume_sparse=True) over a dense key range, finished on the device: the
 * occupied cells of the count(*) grid slice `counts` (range cells, count_isz-byte integers;
 * cell j is key vmin + j; m of them occupied), ordered by the row each key first appears at
 * (the ordered_set grouper's order, groupby.py:97-168), each of ncols device columns src[c]
 * (the aggregators' grid slices, isz[c]-byte items) gathered in that order into the host
 * buffer dst[c] (m items), and the keys written to labels (m items of label_isz bytes). */
int vh_dense_first_take(const void *keys, uint64_t n, int loc, int key_dtype, int64_t vmin, uint64_t range,
                        const void *counts, int count_isz, uint64_t m, int ncols, const void *const *src,
                        const int *isz, void *const *dst, int label_isz, void *labels);
/* host: dsts[c][i] = srcs[c][idx[i]] for ncols columns of itemsizes[c] (1/2/4/8) bytes, i < n,
 * on up to `threads` threads */
int vh_host_take(int ncols, void *const *dsts, const void *const *srcs, const int *itemsizes, const int64_t *idx,
                 uint64_t n, int threads);

/* ---- index_hash_<dtype>: hash_primitives.hpp:623-900 (key -> first row, + duplicate rows) ---
 * The hash map of DataFrame.join (join.py:124-292).  Key identity is the ordered set's: one
 * NaN entry, one null entry (mask byte set), every other key by bit pattern.  initial_capacity:
 * slots of the first table (a power of two >= 16), 0 = the default (then the table is also
 * sized for the rows of each update before it runs); the table grows as needed. */
typedef struct vh_index vh_index;
int vh_index_create(int dtype, uint64_t initial_capacity, vh_index **out);
int vh_index_destroy(vh_index *index);
/* update(keys[, mask], start_index): row i of the chunk has row number start_index + i.  mask
 * may be NULL (1 = null); select may be NULL, rows with select[i] == 0 are not seen at all.  A
 * key maps to the smallest row it was seen at; its other rows are its duplicates.  nan_value /
 * null_value are the largest NaN / null row over all updates -- one rule for every entry: row
 * numbers decide, not the order of the calls (with rows fed in order this is add_nan / add_null
 * overwriting, :652-660).  mask / select may be host or HBM pointers whatever `loc` says of the
 * keys.  Fails once the index was probed (sealed). */
int vh_index_update(vh_index *index, const void *keys, const uint8_t *mask, const uint8_t *select, uint64_t n,
                    uint64_t start_index, int loc);
/* merge (:850-894): every row `other` has seen is seen by `index` too, under the same row
 * number.  Fails once either was probed (the rows an index has seen are dropped at seal). */
int vh_index_merge(vh_index *index, vh_index *other);
/* length = regular rows indexed (distinct keys + duplicate rows) + 1 if any NaN + 1 if any
 * null (:636-645); nan_value / null_value are -1 when absent */
int vh_index_info(vh_index *index, int64_t *length, int64_t *nan_count, int64_t *null_count, int64_t *nan_value,
                  int64_t *null_value, int *has_duplicates);
/* map_index / map_index_with_mask (:679-754): out[i] = first row of keys[i]; nan_value for NaN
 * keys, null_value for mask[i] != 0 (mask may be NULL), -1 for unknown keys (and for NaN / null
 * keys when the index holds none).  *found_unknown = 1 when any -1 was written.  out_itemsize 4
 * or 8; 4 only while every row number is below 2^31.  The first probe seals the index. */
int vh_index_map_index(vh_index *index, const void *keys, const uint8_t *mask, uint64_t n, int loc, void *out,
                       int out_itemsize, int out_loc, int *found_unknown);
/* map_index_duplicates (:756-848), in two calls.  With left_out = right_out = NULL: for every
 * left row whose key has duplicate rows, one pair (start_index + i, duplicate row) per
 * duplicate, in left-row order, duplicates ascending within a key (NaN and masked keys are
 * skipped); the pairs stay in the library and *n_out is their number.  A second call with
 * left_out / right_out (n_out items each, host or HBM; the other arguments are ignored) copies
 * them out and drops them. */
int vh_index_map_index_duplicates(vh_index *index, const void *keys, const uint8_t *mask, uint64_t n,
                                  uint64_t start_index, int loc, uint64_t *n_out, int64_t *left_out, int64_t *right_out);
/* device gather: dsts[c][i] = idx[i] >= 0 ? srcs[c][idx[i]] : 0 for ncols columns of
 * itemsizes[c] (1/2/4/8) bytes, i < n; idx_itemsize 4 or 8 (signed); mask_out (may be NULL):
 * mask_out[i] = idx[i] < 0.  Every buffer is in HBM; non-negative indices must be in range.
 * Eight columns share one pass over idx. */
int vh_take(int ncols, void *const *dsts, const void *const *srcs, const int *itemsizes, const void *idx,
            int idx_itemsize, uint64_t n, uint8_t *mask_out);
/* the inner join's compaction (join.py:215-220): the positions i with idx[i] >= 0, ascending,
 * into left_rows_out (int64) and their idx[i] into idx_out (idx_itemsize bytes each); both
 * have room for n items, *m are written.  Every buffer is in HBM. */
int vh_index_matched(const void *idx, int idx_itemsize, uint64_t n, uint64_t *m, int64_t *left_rows_out, void *idx_out);

/* ---- multi-GPU (comm.hip): RCCL bound by the library, one process per GPU ----------
 * The reference has no multi-process path; its ExecutorLocal reduces per-thread task
 * parts serially (execution.py:285, Aggregator::reduce superagg.cpp:160-167,205-212,
 * 252-259,354-361,470-480).  Across GPUs the same reductions run as collectives on the
 * library stream.  The caller distributes rank 0's unique id (128 bytes)
 * to every rank before vh_comm_init (vaex_amd/comm.py does it over its host channel). */
typedef struct vh_comm vh_comm;
int vh_comm_unique_id(void *out128);
int vh_comm_init(const void *id128, int world, int rank, vh_comm **out); /* on the current device;
  every vh_comm_* call (and vh_hashagg_exchange) runs on that device, from any thread */
/* `world` loopback ranks in this process on the current GPU, out[0..world): one host
 * thread per rank calls the same collectives (a rendezvous; the last thread to arrive moves
 * every rank's bytes with device copies, all-reduce = all-gather + rank-order device fold).
 * A test backend: the device code around the collectives runs with N ranks' data on one
 * GPU, where RCCL refuses two ranks on one device.  Destroy each handle. */
int vh_comm_loopback(int world, vh_comm **out);
int vh_comm_destroy(vh_comm *comm);
/* in-place all-reduce of `count` items of `dtype` (host or HBM buffer) with vh_op */
int vh_comm_allreduce(vh_comm *comm, void *buf, uint64_t count, int dtype, int op, int loc);
/* recv = every rank's `bytes` of send, rank-major */
int vh_comm_allgather(vh_comm *comm, const void *send, void *recv, uint64_t bytes, int loc);
/* send / recv hold per-rank segments back to back in rank order (sizes in bytes) */
int vh_comm_alltoallv(vh_comm *comm, const void *send, const uint64_t *send_bytes, void *recv,
                      const uint64_t *recv_bytes, int loc);
int vh_comm_barrier(vh_comm *comm);
/* an aggregator's HBM grid combined across ranks in place: SUM for count / sum / moment,
 * MIN / MAX for min / max, AggFirst by (order, rank) on the device (superagg.cpp:470-480) */
int vh_comm_agg_allreduce(vh_comm *comm, vh_agg *agg);
/* groupby results across ranks (after vh_hashagg_finish): every group row to its owner
 * rank splitmix64(key bits) % world over RCCL, owners fold equal keys in rank order; with
 * `gather` every rank then holds the whole key-sorted result (read with vh_hashagg_read) */
int vh_hashagg_exchange(vh_hashagg *h, vh_comm *comm, int gather);

/* ---- expressions on HBM columns (expr.hip) ----------------------------------
 * out[i] = program(cols[.][i]) for i < n: the device evaluation of a virtual column,
 * selection or filter (the reference evaluates them with numpy per chunk, cpu.py:542-581,
 * execution.py:337-341).  code: stack program compiled by vaex_amd/expr.py (op | arg << 8),
 * consts: 64-bit constant bit patterns; HBM columns and output.  Three program shapes run a
 * kernel of their own, 8 rows per lane, with results identical to the interpreter's: a
 * conjunction / disjunction of column-constant comparisons (VH_EXPR_TERMS=0 turns it off),
 * COL DT_FIELD (VH_EXPR_DTFIELD=0), and COL(1-byte mask) CONST COL(data) WHERE with 4- or 8-byte
 * items and the data column's dtype as the result's: fillmissing(column, constant)
 * (VH_EXPR_FILL=0); each switch is read per call. */
int vh_expr_eval(const uint32_t *code, int ncode, const uint64_t *consts, int nconsts, const void *const *cols,
                 const int *col_dtypes, int ncols, uint64_t n, int out_dtype, void *out);

/* ---- selections on HBM columns (select.hip) ---------------------------------
 * how a selection combines with the one before it (selections.py:11-36 _select_functions);
 * with no previous mask and / or / xor give the new mask and subtract its complement */
enum vh_select_mode {
    VH_SELECT_REPLACE = 0, VH_SELECT_AND = 1, VH_SELECT_OR = 2, VH_SELECT_XOR = 3, VH_SELECT_SUBTRACT = 4
};
/* The lasso (SelectionLasso.evaluate, selections.py:172-204, over vaexfast.cpp:1757-1775
 * pnpoly): mask[i] = mode(prev[i] == 1, inside(x[i], y[i])) as 0 / 1 bytes; prev may be NULL.
 * x / y: HBM columns of float64 or float32 (each its own dtype), read as float64; prev / out:
 * HBM, out may be prev.  vertx / verty: host arrays of nvert >= 0 vertices (nvert = 0: nothing
 * is inside); only they are copied to the device, and nothing is read back.  inside() is the
 * reference's arithmetic in float64, operation for operation (IEEE division, no contraction):
 *   d = (tx-meanx)*(tx-meanx) + (ty-meany)*(ty-meany);  inside = 0 unless d < radius*radius
 *   for i, j = i-1 (j = nvert-1 for i = 0):
 *     if ((vy[i] > ty) != (vy[j] > ty)) && (tx < (vx[j]-vx[i]) * (ty-vy[i]) / (vy[j]-vy[i]) + vx[i])  c = !c
 * so the mask equals the C loop's bit for bit (NaN / inf coordinates are never inside).
 * VH_ERR_ARG: another dtype, nvert < 0, an unknown mode, a null column with n > 0. */
int vh_pnpoly(const void *x, int x_dtype, const void *y, int y_dtype, uint64_t n, const double *vertx,
              const double *verty, int nvert, double meanx, double meany, double radius, const uint8_t *prev, int mode,
              uint8_t *out);
/* out = mode(a == 1, b == 1) as 0 / 1 bytes; b NULL: out = !(a == 1).  HBM buffers; out may be
 * a or b.  Only bytes equal to 1 count as selected, as everywhere in the engine. */
int vh_mask_combine(const uint8_t *a, const uint8_t *b, int mode, uint64_t n, uint8_t *out);

/* ---- missing-value masks of HBM columns (missing.hip) ---------------------------
 * A missing mask is one uint8 per row, 1 = missing (numpy's convention, the one
 * vh_binner_set_data_mask / vh_agg_set_data_mask take).  Every buffer is in HBM.
 * vh_mask_unpack_bits: an Arrow validity bitmap (bit i of byte i / 8, LSB first, 1 = valid) to a
 * byte mask: out[i] = !bit(bit_offset + i) for i < n.  bits holds (bit_offset + n + 7) / 8 bytes;
 * nothing past them is read.  One lane per 8 rows, one 8-byte store (byte stores for a ragged
 * tail or a destination that is not 8-aligned).
 * vh_mask_pack_bits: the reverse at bit offset 0: bit i of out_bits = (mask[i] == 0), the padding
 * bits of the last of its (n + 7) / 8 bytes 0.  Any non-zero mask byte is missing.
 * vh_mask_count: *count = the number of non-zero bytes of mask[0 .. n) (synchronises).
 * VH_ERR_ARG: a null or host buffer with n > 0. */
int vh_mask_unpack_bits(const uint8_t *bits, uint64_t bit_offset, uint64_t n, uint8_t *out);
int vh_mask_pack_bits(const uint8_t *mask, uint64_t n, uint8_t *out_bits);
int vh_mask_count(const uint8_t *mask, uint64_t n, uint64_t *count);

/* combined int64 key of a multi-key groupby, out[i] = sum_j (cols[j][i] - mins[j]) * mults[j]
 * (the cartesian ordinal of groupby.py:248-288 _combine, first key most significant);
 * HBM columns and output, up to 8 integer key columns */
int vh_combine_keys(uint64_t n, int nkeys, const void *const *cols, const int *dtypes, const int64_t *mins,
                    const int64_t *mults, int64_t *out);

/* dense rank of an int64 HBM column: rank[i] = number of distinct keys below keys[i], the
 * distinct keys ascending in distinct[0..*m) (capacity n); n < 2^31.  Replaces the
 * GrouperCombined set of a combined key (groupby.py:248-288, ordered_set::create +
 * map_ordinal, hash_primitives.hpp:468-516,543-583) with sorted ordinals. */
int vh_dense_rank_i64(uint64_t n, const int64_t *keys, int32_t *rank, int64_t *distinct, uint64_t *m);

/* ---- row order on HBM columns (sort.hip) ---------------------------------------
 * The kept rows of a byte mask (the reference's mask.first(k)): the positions i < n with
 * mask[i] != 0, ascending, into rows_out (signed, out_itemsize 4 or 8 bytes each; 4 only while
 * n < 2^31), which has room for n items; *m are written.  Every buffer is in HBM. */
int vh_mask_rows(const uint8_t *mask, uint64_t n, int out_itemsize, void *rows_out, uint64_t *m);
/* Stable argsort of 1 to 16 HBM key columns of n rows (keys[k] of dtypes[k], the first key the
 * most significant): DataFrame.sort (dataframe.py:4420-4461) and the Grouper sort=True order
 * (groupby.py:137-156).  rows == NULL: every row (m must equal n); else rows is an ascending
 * list of m row numbers (what vh_mask_rows writes) and only those rows are sorted.  perm_out
 * takes m row numbers of the columns, so one vh_take finishes a sort; rows and perm_out hold
 * signed items of rows_itemsize bytes (4 only while n < 2^31) in HBM.
 * The order is np.lexsort(keys[::-1]) over those rows (one key: np.argsort(kind="stable")):
 * stable, NaN after every number and all NaN equal, -0.0 == 0.0.  descending != 0: the exact
 * reverse of that order (tied rows in reverse row order).
 * VH_ERR_ARG: a row number in rows outside [0, n) (nothing is written then). */
int vh_argsort(int nkeys, const void *const *keys, const int *dtypes, uint64_t n, const void *rows, int rows_itemsize,
               uint64_t m, int descending, void *perm_out);

/* group labels of combined keys (the inverse of vh_combine_keys; groupby.py:248-288 decodes
 * the GrouperCombined bins back to per-key labels): v = table ? table[ck[i]] : ck[i],
 * outs[j][i] = (v / mults[j]) % spans[j] + mins[j] stored in itemsizes[j] bytes; HBM buffers */
int vh_decode_keys(uint64_t n, const int64_t *ck, const int64_t *table, int nkeys, const int64_t *mins,
                   const int64_t *mults, const int64_t *spans, const int *itemsizes, void *const *outs);

/* ---- string columns in HBM (strings.hip) -------------------------------------------
 * A string column is the Arrow layout: n + 1 offsets (int32 or int64, off_itemsize 4 or 8) into
 * a byte buffer.  The byte buffer's allocation starts 8-aligned and carries at least 16 bytes
 * after its last byte; a slice passes its own offsets pointer and the parent's bytes.  Every
 * entry but the check itself takes offsets that passed it.
 *
 * The check: *bad = 0 when the n + 1 offsets are non-negative, non-decreasing and the last is
 * at most nbytes; else bit 0: a negative offset, bit 1: a decreasing pair, bit 2: the last
 * offset past the buffer.  Reads no bytes. */
int vh_str_validate(const void *offsets, int off_itemsize, uint64_t n, uint64_t nbytes, int *bad);
/* out[i] = the length of row i in bytes (kind 0) or in UTF-8 code points (kind 1: the bytes
 * that are not 10xxxxxx) */
int vh_str_len(const void *offsets, int off_itemsize, const uint8_t *bytes, uint64_t n, int kind, int64_t *out);
/* out[i] = 0 / 1: row i against a literal pattern (a host buffer of at most 1024 bytes).
 * op 0: equal, 1: not equal, 2: starts with, 3: ends with, 4: contains (an empty pattern is
 * contained in every string) */
int vh_str_match(const void *offsets, int off_itemsize, const uint8_t *bytes, uint64_t n, int op, const uint8_t *pattern,
                 uint64_t pattern_len, uint8_t *out);
/* The gather column[indices] in two calls, so that the caller can size the output in between.
 * The plan: pos[0 .. m] (HBM) = the exclusive scan of the taken rows' byte lengths, *total the
 * sum.  indices: m row numbers (HBM, int32 or int64) of a column of n rows; a row number outside
 * [0, n) takes the empty string. */
int vh_str_take_plan(const void *offsets, int off_itemsize, uint64_t n, const void *indices, int idx_itemsize, uint64_t m,
                     uint64_t *pos, uint64_t *total);
/* the copy: out_offsets (m + 1 of out_itemsize bytes; 4 only while total < 2^31) and out_bytes
 * (total bytes + 16 of slack) from the plan */
int vh_str_take(const void *offsets, int off_itemsize, const uint8_t *bytes, uint64_t n, const void *indices,
                int idx_itemsize, uint64_t m, const uint64_t *pos, uint64_t total, void *out_offsets, int out_itemsize,
                uint8_t *out_bytes);
/* String-producing functions of a column, in two calls like the gather: the
 * plan writes pos[0 .. n] (HBM), the exclusive scan of the rows' result lengths, and *total;
 * the write fills out_offsets (n + 1 of out_itemsize bytes; 4 only while total < 2^31) and
 * out_bytes (total bytes + 16 of slack).  Both calls take the same op and parameters.
 * op 0: lower, 1: upper (flags 1: ASCII letters only; else table holds ntable <= 2048 pairs
 * (code point, image), sorted, none below 128: the host's case table), 2: slice [a, b) in code
 * points (flags 1: b is given), 3: strip the ASCII bytes c0[0 .. n0) (flags 1: left, 2: right,
 * 3: both), 4: pad to a code points with the byte c0[0] (flags as strip: the side(s) that grow),
 * 5: repeat a times, 6: cat with the constant c0 (flags 1: the constant first) or with the same
 * row of a second column (offsets2 / bytes2, flags 2), 7: replace c0 (not empty) by c1, at most
 * a times (a < 0: all).  Constants are host buffers of at most 1024 bytes; offsets2 is NULL
 * unless op is 6 with flags 2.  Repeats and widths are any int64: when a row's result, or the
 * sum, cannot fit (a row above 2^62 / (n + 1) bytes) the plan sets *total to
 * VH_STR_FN_TOO_LONG, and no write may follow. */
#define VH_STR_FN_TOO_LONG UINT64_MAX
int vh_str_fn_plan(const void *offsets, int off_itemsize, const uint8_t *bytes, uint64_t n, const void *offsets2,
                   int off2_itemsize, const uint8_t *bytes2, int op, int64_t a, int64_t b, int flags, const uint8_t *c0,
                   uint64_t n0, const uint8_t *c1, uint64_t n1, const uint32_t *table, uint64_t ntable, uint64_t *pos,
                   uint64_t *total);
int vh_str_fn(const void *offsets, int off_itemsize, const uint8_t *bytes, uint64_t n, const void *offsets2, int off2_itemsize,
              const uint8_t *bytes2, int op, int64_t a, int64_t b, int flags, const uint8_t *c0, uint64_t n0,
              const uint8_t *c1, uint64_t n1, const uint32_t *table, uint64_t ntable, const uint64_t *pos, uint64_t total,
              void *out_offsets, int out_itemsize, uint8_t *out_bytes);
/* The dictionary encoder (superutils.ordered_set_string): the distinct strings of the columns
 * it has seen, numbered in first-appearance order, kept in a dictionary of its own in HBM.
 * hash_bits (0 .. 64): the low bits of the 64-bit hash that the slot tables key on; fewer than
 * 64 forces collisions, which the encoder resolves exactly (a test seam).  initial_capacity:
 * slots of a fresh table, 0 for the default. */
int vh_strset_create(int hash_bits, uint64_t initial_capacity, void **out);
int vh_strset_destroy(void *set);
/* add the strings of n < 2^32 rows */
int vh_strset_update(void *set, const void *offsets, int off_itemsize, const uint8_t *bytes, uint64_t n);
int vh_strset_info(void *set, int64_t *count, int64_t *dict_bytes, int64_t *levels, int64_t *table_bytes);
/* the dictionary to the host: count + 1 offsets and dict_bytes bytes */
int vh_strset_dict(void *set, int64_t *offsets_out, uint8_t *bytes_out);
/* out[i] (HBM, int32) = the ordinal of row i, -1 for a string the set does not hold */
int vh_strset_map_ordinal(void *set, const void *offsets, int off_itemsize, const uint8_t *bytes, uint64_t n, int32_t *out);

#ifdef __cplusplus
}
#endif
#endif /* VAEXHIP_H */
