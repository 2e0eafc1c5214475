// mic_internal.h — shared between the HIP kernels and the engine (not part of the public ABI).
#ifndef MIC_INTERNAL_H
#define MIC_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <time.h>

#include "mi_clark.h"

// ---- exact 64-bit division by a runtime-constant divisor (HTSIZE) -------------------------------
// Granlund–Montgomery "round-up" magic, computed once on the host (mic_make_div):
//   magic == 0 : divisor is a power of two, q = n >> shift
//   add == 0   : q = mulhi(magic, n) >> shift
//   add == 1   : q = (((n - t) >> 1) + t) >> shift,  t = mulhi(magic, n)
// Replaces the reference's compile-time-constant division `c / HTSIZE` (CuClarkDB.cu:1268-1269):
// HTSIZE is a runtime value here (= size of .sz), so one binary serves cuCLARK and cuCLARK-l.
struct MicDiv {
  uint64_t d;
  uint64_t magic;
  uint32_t shift;
  uint32_t add;
};

MicDiv mic_make_div(uint64_t d);

#ifdef __cplusplus
#include <vector>
// mic_host.cpp: mic_pack_reads plus, per part, the offset of its first nucleotide in its ACGTU run and the run's length
size_t mic_pack_reads_runs(const uint8_t* map, const uint64_t* seq_s, const uint64_t* seq_e, const uint64_t* length,
                           size_t n_reads, int k, uint32_t* reads_pointer, uint16_t* containers, size_t cap,
                           std::vector<uint64_t>* run_off, std::vector<uint64_t>* run_len);
#endif

static inline __host__ __device__ uint64_t mic_mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

static inline __host__ __device__ uint64_t mic_div(uint64_t n, const MicDiv& dv) {
  if (dv.magic == 0) return n >> dv.shift;
  uint64_t t = mic_mulhi64(dv.magic, n);
  if (dv.add) return (((n - t) >> 1) + t) >> dv.shift;
  return t >> dv.shift;
}

// ---- resident table --------------------------------------------------------------------------
// One 64-byte slot per bucket = 4 quarters of 16 bytes; a quad of 4 lanes loads one slot with a single
// wave-instruction (global_load_dwordx4), i.e. ONE random 64-byte request per probe.
//   slot class 32 (quotients < 2^32; u16/u32 keys on disk): quarter j = { key[2j], key[2j+1],
//        label[2j] | label[2j+1] << 16, meta }        -> 8 entries inline
//   slot class 64 (u64 keys on disk): quarter j = { key_lo, key_hi, label, meta } -> 4 entries inline
//   meta: bits 0..7 = n, entries stored from this slot onwards along the chain (saturating at 255);
//         bits 8..31 of quarters 0 and 1 = low / high 24 bits of the absolute index of the next slot
//         of the chain (used only when n > capacity).
// Entries are the bucket's keys that the reference's linear scan can reach (strict prefix maxima
// that are <= the bucket's last key, CuClarkDB.cu:1291-1307), in ascending order.
#define MIC_SLOT_BYTES 64
#define MIC_FLAG_ROW_OVERFLOW_ 1u  /* == MIC_FLAG_ROW_OVERFLOW */
#define MIC_FLAG_DENSE_PATH_ 2u    /* == MIC_FLAG_DENSE_PATH   */
#define MIC_ROW_INVALID 0xFFFFFFFFu     /* row[0] of a sparse row that did not fit */
#define MIC_CAP32 8
#define MIC_CAP64 4

// ---- minimizer-keyed table ("M-table", layout 1) ---------------------------------------------------------------
// A k-mer's slot is chosen by the smallest 32-bit order key among its w = k-m+1 canonical m-mers (mic_device.h), so
// the ~ (w+1)/2 consecutive k-mers of a read that share a minimizer share ONE slot: the query kernel loads each
// distinct slot of a 128-k-mer chunk once from HBM into LDS (8 lanes x 16 B) and every k-mer compares against the
// staged entries.  Slots hold full canonical k-mers, so membership and labels are exact.
//   128-byte slot: keys u64[12] (ascending along the chain, unused = ~0) | labels u16[12] | meta u32 | next u32
//   meta: bits 0..7 = entries in this slot, bit 8 = chain continues at slot `next` (overflow slots are contiguous)
#define MIC_MCAP 12
#define MIC_MSLOT_BYTES 128
#ifndef MIC_LAYOUT_MINIMIZER
#define MIC_LAYOUT_AUTO 0
#define MIC_LAYOUT_DIRECT 1
#define MIC_LAYOUT_MINIMIZER 2
#endif
#ifndef MIC_LAYOUT_SUPER
#define MIC_LAYOUT_SUPER 3
#endif
#ifndef MIC_LAYOUT_SUPER2
#define MIC_LAYOUT_SUPER2 4
#endif

struct MicTable {
  const uint4* slots;    // layout 0: 4 x uint4 per slot; layout 1: 8 x uint4 per slot
  uint64_t n_main;       // layout 0: shard_end - shard_start; layout 1: number of main M-slots
  uint64_t shard_start;  // first bucket of the shard
  uint64_t shard_end;
  MicDiv div;            // division by htsize
  int k;
  int layout;            // 0 = direct slots, 1 = minimizer-keyed slots, 2 = super-k-mer slots
  int m;                 // minimizer length (layout 1)
  int sharded;           // 1 if [shard_start, shard_end) is a strict subset of the table
  int fwd;               // layout 2: both strands stored under forward-strand minimizers (mic_device.h: s_candidates_fwd)
  // layout 2, slot-range part (table-sharded runs): only the main slots [slot_lo, slot_lo + slot_cnt) of the n_main the
  // minimizer hash spreads over are resident; `slots` is then the allocation MINUS slot_lo slots, so global slot indices
  // (and the continuation indices stored in word 31) address it directly.  slot_cnt == 0: the whole table is here.
  uint32_t slot_lo, slot_cnt;
  // layout 2: the k-mers of crowded minimizers, keyed by the oriented k-mer: cells {lo, hi, label + 1, 0}, label + 1 == 0 is
  // empty, linear probing, side_mask + 1 cells (a power of two); null when the table has none
  const uint4* side; uint32_t side_mask;
  int parted;            // 1: slot-range part as above (slot_cnt may be 0: an empty part answers nothing)
  const uint8_t* sizes;  // kept copy of the shard's on-disk bucket sizes (statistics only)
};

struct MicQueryArgs {
  MicTable t;
  const uint32_t* reads_ptr;
  const uint16_t* cont;
  uint32_t n_reads;
  uint32_t row_words;   // 0 => no rows
  uint32_t* results;    // n_reads * 8
  uint32_t* rows;       // n_reads * row_words or nullptr
  uint32_t* flagged;    // [0] = count, [1..] = read ids needing the dense path (or nullptr)
  uint32_t flagged_cap;
  // layout 2 with a side table: the work area through which query_kernel_r hands the runs of crowded minimizers (and the rows
  // of their reads) to crowd_finish_kernel - mic_crowd_dims / mic_crowd_attach below - or nullptr: such reads take the dense path
  uint32_t* crowd;
  uint32_t* crowd_items; uint32_t* crowd_pool;      // = crowd + MIC_CROWD_HDR + 8 pend_cap, ... + 8 item_cap (the kernels do no address arithmetic with the capacities)
  uint32_t crowd_pend_cap, crowd_item_cap, crowd_pool_cap;
};

// ---- work area of the crowded runs' follow-up (mic_kernels.hip: query_kernel_r -> crowd_finish_kernel) ----------------------
// One per query launch in flight, any 16-byte aligned device memory; mic_launch_query zeroes the header.  Words:
//   [0] pending reads  [1] items  [2] pool words  [3] reads sent to the dense path for lack of room  [4..7] unused
//   pending read p (8 words): read, hits so far, entries | overflow << 8 (0xFFFFFFFF: skipped), pool offset of its row, last group
//   item i (8 words): the run's region (3 words, oriented as the table stores it), jmin | jmax << 8, the group in front (first item of a group)
//   pool: the rows so far, (label + 1, count) per entry
// A group = the crowded runs of one round of one read, adjacent items: first item | (runs - 1) << 27.
#define MIC_CROWD_HDR 8
#define MIC_CG_NONE 0xFFFFFFFFu
#define MIC_CG_DENSE 0xFFFFFFFEu
struct MicCrowdDims { uint32_t pend_cap, item_cap, pool_cap; size_t words; };
static inline MicCrowdDims mic_crowd_dims(size_t max_reads) {
  // a quarter of the reads pending with four crowded runs and eight row words each (48 bytes per read of capacity); what does
  // not fit takes the dense path (exact, slow: real data has a few per cent of such reads, a run or two each)
  MicCrowdDims d;
  const size_t cap27 = (1u << 27) - 64;
  size_t pend = max_reads / 4 + 1024, item = max_reads + 4096, pool = max_reads * 2 + 8192;
  d.pend_cap = (uint32_t)(pend < cap27 ? pend : cap27);
  d.item_cap = (uint32_t)(item < cap27 ? item : cap27);
  d.pool_cap = (uint32_t)(pool < 0xFFFFFF00u ? pool : 0xFFFFFF00u);
  d.words = MIC_CROWD_HDR + 8 * ((size_t)d.pend_cap + d.item_cap) + d.pool_cap;
  return d;
}
static inline void mic_crowd_attach(MicQueryArgs& a, uint32_t* area, size_t max_reads) {
  const MicCrowdDims d = mic_crowd_dims(max_reads);
  a.crowd = area; a.crowd_pend_cap = area ? d.pend_cap : 0; a.crowd_item_cap = area ? d.item_cap : 0; a.crowd_pool_cap = area ? d.pool_cap : 0;
  a.crowd_items = area ? area + MIC_CROWD_HDR + 8 * (size_t)d.pend_cap : nullptr;
  a.crowd_pool = area ? a.crowd_items + 8 * (size_t)d.item_cap : nullptr;
}

// stage times of the table build in progress (mic_engine.hip; read back with mic_db_last_build_report)
void mic_build_report_add(const char* what, double seconds);
// device memory the engine's caller is allocating concurrently with the build (mic_db_reserve_hbm): not available to it
extern thread_local uint64_t mic_build_reserved_hbm;

// launchers (mic_kernels.hip)
hipError_t mic_launch_query(const MicQueryArgs& a, int slot_class, int n_cu, hipStream_t s);
// name of the instantiation mic_launch_query picks for this table, as a kernel trace shows it; returns the length
int mic_query_kernel_name(const MicTable& t, int slot_class, char* buf, size_t cap);
hipError_t mic_kernels_warm(hipStream_t s);      // loads the query kernels' device code (a no-op kernel of their file)
hipError_t mic_launch_merge_rows(const uint32_t* a, const uint32_t* b, uint32_t* out, uint32_t row_words, size_t n,
                                 uint32_t* flags_results, hipStream_t s);
hipError_t mic_launch_result_from_rows(const uint32_t* rows, uint32_t row_words, uint32_t* results, size_t n,
                                       hipStream_t s);
hipError_t mic_launch_dense_count(const MicTable& t, int slot_class, const uint32_t* reads_ptr, const uint16_t* cont,
                                  const uint32_t* ids, size_t n_ids, uint32_t n_targets, uint32_t* counts,
                                  hipStream_t s);
hipError_t mic_launch_dense_finish(const uint32_t* counts, const uint32_t* ids, size_t n_ids, uint32_t n_targets,
                                   uint32_t* results, uint32_t* rows, uint32_t row_words, hipStream_t s);

hipError_t mic_launch_probe_stats(const MicTable& t, int slot_class, const uint32_t* reads_ptr, const uint16_t* cont,
                                  size_t n_reads, unsigned long long* d_out, hipStream_t s);

// table build (mic_build.hip)
struct MicBuildOut {
  uint4* slots;
  uint64_t n_main, n_overflow, n_elems, n_elems_file;
  uint32_t max_bucket;
  uint32_t max_chain;   // layout 1: entries in the fullest slot chain
  uint32_t walk_ppm;    // super-k-mer table: mean continuation slots in front of a stored k-mer, x 1e6
  uint64_t n_entries;   // super-k-mer table: entries (super-k-mers) stored; other layouts: 0 (= one entry per k-mer)
  uint4* side; uint64_t side_cells, side_kmers;   // super-k-mer table: the k-mers of crowded minimizers (mic_build.hip: s_crowd_move_kernel), or null
  uint64_t part_lo, part_hi; // super-k-mer table built as a slot-range part: the main slots [part_lo, part_hi) of n_main are resident (else 0, n_main)
  uint64_t alloc_slots; // slots allocated when that is more than n_main + n_overflow + 1 (one-pass super-k-mer build: the unused part of its continuation pool), else 0
};
// d_sizes/d_keys/d_labels point at the first bucket / first element of the shard.
// rank_base = number of non-empty buckets before the shard (sampling is defined on the whole table).
int mic_build_table(const uint8_t* d_sizes, uint64_t n_buckets, const void* d_keys, int key_bytes,
                    const uint16_t* d_labels, uint32_t sampling, uint64_t rank_base, int slot_class, hipStream_t s,
                    MicBuildOut* out, char* err, size_t err_cap);
// Minimizer-keyed table from the same inputs.  bucket0 = index of the shard's first bucket in the whole table.
int mic_build_mtable(const uint8_t* d_sizes, uint64_t n_buckets, uint64_t bucket0, uint64_t htsize, const void* d_keys,
                     int key_bytes, const uint16_t* d_labels, uint32_t sampling, uint64_t rank_base, int k, int m,
                     hipStream_t s, MicBuildOut* out, char* err, size_t err_cap);
// Super-k-mer table (layout 3, mic_device.h) from the same inputs.
int mic_build_stable(const uint8_t* d_sizes, uint64_t n_buckets, uint64_t bucket0, uint64_t htsize, const void* d_keys,
                     int key_bytes, const uint16_t* d_labels, uint32_t sampling, uint64_t rank_base, int k, int m,
                     hipStream_t s, MicBuildOut* out, char* err, size_t err_cap, int allow_fallback, int both_strands,
                     uint32_t part, uint32_t n_parts);
// (part of n_parts > 1: only the main slots [n_slots * part / n_parts, n_slots * (part + 1) / n_parts) of the table sized for the
// whole input are built; out->slots is the allocation, slot s of the table lives at out->slots + (s - out->part_lo) * 8)
// (allow_fallback: return -5 instead of building a table whose minimizers are crowded: see s_walk_kernel)
// sums over d_sizes[0..n): total elements and non-empty buckets
int mic_reduce_sizes(const uint8_t* d_sizes, uint64_t n, uint64_t* total, uint64_t* nonzero, hipStream_t s);

// Streams and events come from a process-wide pool and go back to it; none is ever destroyed (mic_engine.hip: why).
hipError_t mic_stream_get(hipStream_t* s);                 // a non-blocking stream of the current device
void mic_stream_put(hipStream_t s);                        // drained first; nullptr is fine
hipError_t mic_event_get(hipEvent_t* ev, bool timing);     // an event of the current device
void mic_event_put(hipEvent_t ev);

// ---- abundance counters (mic_abund.hip) ----------------------------------------------------------------------------------------
// An engine's counters while mic_abundance_start is in force: n_words = num_targets + 2 u64 on the engine's device.
struct MicAbund {
  unsigned long long* d_counts = nullptr;
  uint32_t n_words = 0;
  bool on = false;
  uint64_t conf_num = 5, conf_den = 10, gamma_num = 0, gamma_den = 1;
};
// adds reads [0, n) of `results` to `counts` by the rule of mic_abund.h: norm of read r = norm[r] - norm_sub (norm == nullptr: 0);
// status != nullptr: a non-zero *status (the batch is handed back) makes the launch add nothing
hipError_t mic_launch_abund(const uint32_t* results, const uint32_t* norm, uint32_t norm_sub, size_t n, int k, uint32_t n_targets,
                            const MicAbund& f, unsigned long long* counts, const uint32_t* status, hipStream_t s);

// ---- score-density counters (mic_density.hip; the rule: mic_density.h) -----------------------------------------------------------
// An engine's counters while mic_density_start is in force: MIC_DENSITY_WORDS u64 on the engine's device.
struct MicDensity {
  unsigned long long* d_counts = nullptr;
  bool on = false;
};
// adds reads [0, n) of `results` to `counts` (MIC_DENSITY_WORDS u64) by the rule of mic_density.h; norm, norm_sub and status as for
// mic_launch_abund; n_cu caps the grid
hipError_t mic_launch_density(const uint32_t* results, const uint32_t* norm, uint32_t norm_sub, size_t n, int k, uint32_t n_targets,
                              int n_cu, unsigned long long* counts, const uint32_t* status, hipStream_t s);

// ---- k-mer sketches (mic_ksketch.hip; the kernel: mic_kernels.hip; the rule: mic_ksketch.h) ----------------------------------------
// An engine's sketches while mic_ksketch_start is in force: one allocation on the engine's device, n_targets * MIC_KSKETCH_REGS
// register bytes followed by n_targets u64 hit counters.
struct MicKsketch {
  uint8_t* d_regs = nullptr;
  unsigned long long* d_hits = nullptr;
  uint32_t n_targets = 0;
  bool on = false;
};
// adds the k-mers of reads [0, n_reads) whose table label is a target to regs (max) and hits (sum) by the rule of mic_ksketch.h; a
// read whose result row has sum 0 is skipped; regs 4-byte aligned; status as for mic_launch_abund; n_cu caps the grid
hipError_t mic_launch_ksketch(const MicTable& t, int slot_class, int n_cu, const uint32_t* reads_ptr, const uint16_t* cont, size_t n_reads,
                              const uint32_t* results, uint32_t n_targets, uint8_t* regs, unsigned long long* hits, const uint32_t* status,
                              hipStream_t s);

// ---- hit maps (mic_hitmap.hip; the kernel: mic_kernels.hip; the text kernels: mic_ingest.hip; the rule: mic_hitmap.h) ----------------
// An engine's setting while mic_hitmap_start is in force: every ingest batch it owns that returns MIC_INGEST_OK gets its map and text.
// kraken: the text is Kraken's per-read line (mic_kraken_start; the rule: mic_kraken.h) instead of the hit-map line - the same two probe
// passes, the same slot buffers, another pair of text kernels; a run has one text or the other.
struct MicHitmap {
  bool on = false;
  bool kraken = false;
  mic_abund_filter filter = {5, 10, 0, 1};
};
// one pass of hitmap_kernel over reads [0, n_reads): fill == false: out = n_reads + 1 word counts (item n_reads = 0), offsets unused;
// fill == true: out = the words, offsets = the exclusive sum of the counts (n_reads + 1).  n_cu caps the grid.
hipError_t mic_launch_hitmap(const MicTable& t, int slot_class, int n_cu, const uint32_t* reads_ptr, const uint16_t* cont, size_t n_reads,
                             const uint32_t* results, uint32_t n_targets, const uint32_t* offsets, uint32_t* out, bool fill, hipStream_t s);
// the scan between the passes: its temporary storage for n_items u32, and the scan itself (counts -> offsets)
size_t mic_hitmap_tmp_bytes(size_t n_items);
hipError_t mic_hitmap_scan(void* d_tmp, size_t tmp_bytes, const uint32_t* counts, uint32_t* offsets, size_t n_items, hipStream_t s);
// count, scan, word total to the host, fill when the words fit cap_words (mic_hitmap_device's contract) on device arrays; synchronous
int mic_hitmap_run(const MicTable& t, int slot_class, int n_cu, const uint32_t* d_rp, const uint16_t* d_cont, size_t n_reads,
                   const uint32_t* d_results, uint32_t n_targets, uint32_t* d_offsets, uint32_t* d_words, size_t cap_words, uint64_t* n_words,
                   hipStream_t s);

// ---- the line indexer (mic_text.hip): bytes -> line ends per tile -> line starts ----------------------------------------------------
// One text at a time, all work on stream s, nothing waits.  raw is 16-byte aligned (the kernels load 16 aligned bytes a thread) and
// the text is its bytes [from, nb): an ingest slot's batch and the inflater's texts (mic_pairs_index_device) start at raw, from = 0;
// a text at any other address counts from the 4-KiB boundary below it (mic_text_index_device).
#define MIC_LINE_TILE 4096
static inline uint32_t mic_line_tiles(uint32_t nb) { return (nb + MIC_LINE_TILE - 1) / MIC_LINE_TILE; }
size_t mic_line_scan_bytes(size_t n_tiles);      // the scan storage mic_line_ends needs for a text of n_tiles tiles
// line ends: d_tile[i] = the '\n' of tile i, d_tile_off = their exclusive sum (mic_line_tiles(nb) + 1 entries each, the last one the total)
hipError_t mic_line_ends(const uint8_t* raw, uint32_t nb, uint32_t from, uint32_t* d_tile, uint32_t* d_tile_off, void* d_scan, size_t scan_bytes,
                         hipStream_t s);
// line starts: d_line_start[L] = offset from raw of the first byte of line L, for L < cap (line 0 starts at `from`)
hipError_t mic_line_starts(const uint8_t* raw, uint32_t nb, uint32_t from, const uint32_t* d_tile_off, uint32_t* d_line_start, uint32_t cap,
                           hipStream_t s);
hipError_t mic_text_warm(hipStream_t s);         // loads the device code of mic_text.hip (a no-op kernel of that file)

// ---- table census (the kernel: mic_kernels.hip; the rule: mic_census.h; the engine's side: mic_engine.hip) -------------------------------
// An engine's census while mic_db_census_enable is in force: allocated by the load that runs it (num_targets * 8 + 64 bytes on the
// engine's device: the counts, then the 8 stats), freed by mic_db_unload / mic_destroy; mic_db_census_fetch reads the host copies.
struct MicCensus {
  bool on = false, have = false;          // enabled; the loaded table was counted
  unsigned long long* d_counts = nullptr; // u64[n_targets], then u64[8]
  std::vector<uint64_t> counts;
  uint64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};
// per 256-bucket tile of d_sizes the elements and the non-empty buckets in front of it (mic_build.hip: the builders' pass A), in a
// device allocation the caller frees; 0, -1 (no or too many buckets), -3 (no memory), -4 (HIP error).  Synchronizes s.
int mic_tile_bases(const uint8_t* d_sizes, uint64_t n_buckets, void** d_bases, hipStream_t s);
hipError_t mic_launch_census(const MicTable& t, int slot_class, const uint8_t* d_sizes, uint64_t n_buckets, uint64_t bucket0, uint64_t htsize,
                             const void* d_keys, int key_bytes, const uint16_t* d_labels, const void* bases, uint32_t sampling, uint64_t rank_base,
                             uint32_t n_targets, unsigned long long* counts, unsigned long long* stats, hipStream_t s);

// ---- read splitting (mic_split.hip; the rule: mic_split.h) --------------------------------------------------------------------------
// An engine's setting while mic_split_start is in force: every ingest batch it owns that returns MIC_INGEST_OK is partitioned.
struct MicSplit {
  bool on = false;
  int which = 0;                    // MIC_SPLIT_CLASSIFIED | MIC_SPLIT_UNCLASSIFIED
  mic_abund_filter filter = {5, 10, 0, 1};
};
// work arrays of one launch: n + 1 u64 each (scan input and output), one u32 counter, the scan's temporary storage
struct MicSplitBufs {
  unsigned long long* d_len2 = nullptr; unsigned long long* d_off2 = nullptr; uint32_t* d_ncls = nullptr;
  void* d_tmp = nullptr; size_t tmp_bytes = 0;
};
size_t mic_split_tmp_bytes(size_t n_items);
// partitions the n records of text[0, nb) into out[0, nb + 1): record r begins at starts[r] - start_sub (the last one ends at nb), its
// class comes from results / norm / norm_sub as in mic_launch_abund.  Afterwards b.d_off2[n] = a | b << 32 and *b.d_ncls = the number
// of classified records.  text and out 4-byte aligned; status as for mic_launch_abund.
hipError_t mic_launch_split(const uint8_t* text, uint32_t nb, const uint32_t* starts, uint32_t start_sub, const uint32_t* results,
                            const uint32_t* norm, uint32_t norm_sub, uint32_t n, int k, uint32_t n_targets, const mic_abund_filter& f,
                            int which, const MicSplitBufs& b, uint8_t* out, const uint32_t* status, hipStream_t s);

// ---- rank roll-up (mic_rollup.hip; the rule: mic_rollup.h) ------------------------------------------------------------------------
// An engine's lineage (mic_rollup_set) and, while mic_rollup_start is in force, its counters.  The lineage's device arrays are one
// allocation (d_block).
struct MicRollup {
  uint32_t n_levels = 0;            // 0: no lineage set
  uint32_t n_groups[8] = {};        // [0] = num_targets
  uint32_t off[8] = {};             // counter of group g at level l: 2 + off[l] + g
  uint32_t seg_off[8] = {};         // d_seg + seg_off[l]: the n_groups[l] + 1 segment starts of level l (l >= 1)
  uint32_t n_counters = 0;
  void* d_block = nullptr;
  const uint16_t* d_group_of = nullptr;   // [n_levels][T]
  const uint16_t* d_perm = nullptr;       // [n_levels][T]: the targets sorted by their group at level l (stable)
  const uint32_t* d_seg = nullptr;
  unsigned long long* d_counts = nullptr; // n_counters u64 (mic_rollup_start)
  bool on = false;
  mic_abund_filter filter = {5, 10, 0, 1};
};
// rows form: reads [0, n) of `rows` (row_words u32 each) -> rollup (8 u32 each), levels (optional), counts (optional, added to);
// norm of read r = norm[r] - norm_sub (norm == nullptr: 0); status as for mic_launch_abund
hipError_t mic_launch_rollup(const MicRollup& ru, const uint32_t* rows, uint32_t row_words, const uint32_t* norm, uint32_t norm_sub, size_t n,
                             int k, uint32_t n_targets, const mic_abund_filter& f, uint32_t* rollup, uint32_t* levels,
                             unsigned long long* counts, const uint32_t* status, hipStream_t s);

// ---- the engine as the other files of the library see it (mic_engine.hip defines all of this) --------------------------------------
struct mic_engine;
int mic_engine_table(mic_engine* e, MicTable* t, int* slot_class, int* n_cu, int* device, int* k, uint32_t* n_targets);   // slots == nullptr: no database
int mic_set_error(int code, const char* fmt, ...);     // sets the thread's mic_last_error text, returns code
int mic_bind_thread_near_device(int device, int on);   // the calling thread to the CPUs of the device's NUMA node, or back (on == 0); nests
bool mic_peer_enable(int from, int to);                // device `from` reads device `to`'s memory directly; false: copies are staged
void mic_peer_enable_engines(mic_engine* const* engines, size_t n);
hipStream_t mic_engine_stream(mic_engine* e);
void mic_engine_copy_streams(mic_engine* e, hipStream_t* up, hipStream_t* down);
uint32_t mic_engine_row_words(const mic_engine* e);
void** mic_engine_ingest_slot(mic_engine* e);          // the engine keeps one Ingest* (mic_ingest.hip), opaque to it
MicAbund* mic_engine_abund(mic_engine* e);
MicRollup* mic_engine_rollup(mic_engine* e);
MicDensity* mic_engine_density(mic_engine* e);
MicSplit* mic_engine_split(mic_engine* e);
MicKsketch* mic_engine_ksketch(mic_engine* e);
MicHitmap* mic_engine_hitmap(mic_engine* e);
uint32_t* mic_engine_min_quality(mic_engine* e);
uint32_t* mic_engine_low_complexity(mic_engine* e);
// (mic_ingest.hip defines this one) slot `slot_id` of e's ingest slots as mic_text.hip fills it: the slot's text buffer on the device
// and its stream, the size and the device of e's slots; MIC_E_STATE with the error set when e has no such slot
struct MicSlotText { uint8_t* d_raw; hipStream_t stream; size_t max_bytes; int device; };
int mic_ingest_slot_text(mic_engine* e, size_t slot_id, MicSlotText* out);

static inline double now_s() { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec + t.tv_nsec / 1e9; }

// a failed HIP call sets the error text and returns its code / sets rc and jumps to the function's `done` label
#define MIC_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) \
    return mic_set_error(e_ == hipErrorOutOfMemory ? MIC_E_NOMEM : MIC_E_HIP, "%s: %s", #x, hipGetErrorString(e_)); } while (0)
#define MIC_TRY_DONE(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { \
    rc = mic_set_error(e_ == hipErrorOutOfMemory ? MIC_E_NOMEM : MIC_E_HIP, "%s: %s", #x, hipGetErrorString(e_)); goto done; } } while (0)

#endif
