/*
 * mi_clark.h — C ABI of libmi_clark.so: the MI355X (gfx950) k-mer query engine that replaces
 * CuCLARK's CuClarkDB (device DB + query) behind the same caller contract.
 *
 * Plain C types only (pointers, sizes, fixed-width ints): bindable from C, C++, ctypes, cgo, JNI.
 * Every entry point cites the reference interface it replaces, as file:line under
 * Funatiq/cuclark src/.  All functions return MIC_OK (0) or a negative MIC_E_* code and never
 * exit() or print; mic_last_error() returns the message of the last failure on this thread
 * (reference: CUERR/CUMEMERR print + exit(1), CuClarkDB.cu:45-63).
 *
 * Data contract (unchanged from the reference unless stated):
 *   reads in   : readsPointer u32[nReads+1] + readsInContainers u16[]      CuCLARK_hh.hh:1616-1716
 *                (per read: parts; per part: 1 length slot + ceil(len/8) containers, 8 nt per u16,
 *                 first nt in the top bits, A=3 C=2 G=1 T/U=0).  A length slot of 0 ends a read
 *                 early (lets callers over-allocate per read); the reference never emits one.
 *   results out: MIC_RESULT_WORDS u32 per read:
 *                {sum, idxBest, best, idxSecond, second, nTargetsHit, flags, 0}
 *                words 0..4 are resultKernel's {sumN,indexBest,best,index_sBest,s_best}
 *                (CuClarkDB.cu:1421-1471) widened from u16 to u32; indices are target+1, 0 = "NA".
 *   sparse rows: optional, row_words u32 per read: word0 = n, words 1..n = (count<<16 | target) in
 *                ascending target order (the reference's [n,(t,c)*] u16 rows, CuClarkDB.cu:1178-1243,
 *                one pair per word).  A row that does not fit (n > row_words-1 or a count > 65535) has
 *                word0 = MIC_ROW_INVALID and its read carries MIC_FLAG_ROW_OVERFLOW; words 0..4 of its
 *                result are still exact (dense path), per-target counts come from mic_count_dense_device.
 */
#ifndef MI_CLARK_H
#define MI_CLARK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIC_OK 0
#define MIC_E_INVALID (-1)  /* bad argument                                   */
#define MIC_E_IO (-2)       /* file missing / short (reference: read() returns false, CuClarkDB.cu:490-495) */
#define MIC_E_NOMEM (-3)    /* host or device allocation failed              */
#define MIC_E_HIP (-4)      /* HIP runtime error                              */
#define MIC_E_STATE (-5)    /* call out of order (e.g. query before DB load)  */
#define MIC_E_NODEVICE (-6) /* no usable gfx950 device / kernels not loadable */
#define MIC_E_UNSUPPORTED (-7) /* mic_gz_*: an input this path does not take; the caller uses its other path   */

#define MIC_RESULT_WORDS 8
#define MIC_FLAG_ROW_OVERFLOW 1u /* sparse row did not fit; dense path was used */
#define MIC_FLAG_DENSE_PATH 2u   /* read was (re)processed by the dense fallback */

#define MIC_ROW_INVALID 0xFFFFFFFFu
#define MIC_MAX_PART 65528u /* parts longer than this are packed as overlapping sub-parts */

typedef struct mic_engine mic_engine;

typedef struct mic_config {
  int32_t device;       /* HIP device ordinal; -1 = current device                     */
  int32_t k;            /* k-mer length, 2..32                       main.cc:110-114  */
  uint32_t num_targets; /* number of labels T (<= 65535)             dataType.hh:48   */
  uint32_t num_batches; /* batches of the batch API (>=1)            main.cc:220-226  */
  uint32_t row_words;   /* u32 words per sparse row (0 = default 16 => 15 pairs = MAXHITS, parameters.hh:44) */
  uint32_t layout;      /* resident table layout: MIC_LAYOUT_AUTO / _DIRECT / _MINIMIZER / _SUPER / _SUPER2 */
} mic_config;

#define MIC_LAYOUT_AUTO 0      /* super-k-mer table for k >= 24 (minimizer, then direct if it does not fit), else direct; env MIC_LAYOUT=direct|minimizer|super|super2 overrides */
#define MIC_LAYOUT_DIRECT 1    /* one 64-byte slot per on-disk bucket (one HBM request per k-mer) */
#define MIC_LAYOUT_MINIMIZER 2 /* 128-byte slots keyed by the k-mer's minimizer (one HBM request per ~7 k-mers) */
#define MIC_LAYOUT_SUPER 3     /* 128-byte slots of super-k-mers: the k-mers sharing a minimizer occurrence are one entry; one slot per lookup */
#define MIC_LAYOUT_SUPER2 4    /* the same with BOTH strands of every k-mer stored: the query kernel needs no reverse complement (fastest; twice the table) */

typedef struct mic_db_info {
  uint64_t htsize;         /* buckets in the whole table (= size of .sz)               */
  uint64_t shard_start;    /* first bucket resident on this engine                     */
  uint64_t shard_end;      /* one past the last resident bucket                        */
  uint64_t n_elems;        /* elements resident (after sampling / reachability filter) */
  uint64_t n_elems_file;   /* elements the shard holds on disk                         */
  uint64_t n_slots;        /* 64-byte slots in HBM (main + overflow chain)             */
  uint64_t n_overflow;     /* overflow slots                                            */
  uint64_t hbm_bytes;      /* bytes of HBM held by the table                            */
  int32_t key_bytes;       /* width of the keys on disk: 2, 4 or 8                      */
  int32_t slot_class;      /* 32: 8 entries/slot (u32 quotients); 64: 4 entries/slot; 128: minimizer / super-k-mer table */
  uint32_t max_bucket;     /* largest kept bucket                                       */
  uint32_t sampling;
  int32_t layout;          /* MIC_LAYOUT_DIRECT, _MINIMIZER, _SUPER or _SUPER2          */
  int32_t minimizer_len;   /* m (layouts MINIMIZER, SUPER), else 0                      */
  uint32_t max_chain;      /* entries in the fullest slot chain (MINIMIZER, SUPER)      */
  uint32_t reserved;       /* SUPER: mean number of continuation slots in front of a stored k-mer, x 1e6 (crowded minimizers) */
  uint64_t n_entries;      /* entries stored: super-k-mers (SUPER: several k-mers each), else = n_elems */
  uint32_t part, n_parts;  /* mic_db_set_part (0, 0 when the engine holds the whole database)     */
  uint64_t part_slot_lo;   /* SUPER / SUPER2 with a part: the resident main slots [lo, hi) ...     */
  uint64_t part_slot_hi;
  uint64_t n_slots_whole;  /* ... of this many the whole table has (identical on every part)       */
  uint64_t side_kmers;     /* SUPER / SUPER2: k-mers of crowded minimizers (one minimizer value in more than 12 contexts: microsatellites),
                              kept in a side table keyed by the whole k-mer instead of in slot chains */
  uint64_t side_bytes;     /* HBM of that side table (part of hbm_bytes)                            */
} mic_db_info;

/* ---- engine lifetime: CuClarkDB ctor/dtor (CuClarkDB.cu:85-253) -----------------------------
 * mic_destroy waits for the device and frees the engine's memory; its HIP streams and events go back to a pool of the process
 * for the next engine on that device and are never destroyed (the runtime's completion handler races a stream's destruction:
 * DESIGN.md 7). */
int mic_create(const mic_config* cfg, mic_engine** out);
int mic_destroy(mic_engine* e);
/* test hook: {streams ever created, streams in the pool now, events ever created, events in the pool now} of this process */
int mic_debug_stream_pool(uint32_t out[4]);
const char* mic_last_error(void);
/* Number of usable devices (reference: cudaGetDeviceCount loop, CuClarkDB.cu:104-181). */
int mic_device_count(int* count);

/* ---- database: CuClarkDB::read (CuClarkDB.cu:461-808) + swapDbParts (:813-858) --------------
 * Loads <prefix>.sz/.ky/.lb and builds the resident table.  key_bytes 0 => rule of main.cc:274-316.
 * sampling <=1 keeps all buckets, else every sampling-th non-empty bucket (CuClarkDB.cu:497-524).
 * [shard_start, shard_end) selects the bucket range this engine answers for (the reference's
 * m_partPointer ranges, CuClarkDB.cu:566-574, 1272-1274); shard_end 0 => htsize. */
int mic_db_load_files(mic_engine* e, const char* prefix, int key_bytes, uint32_t sampling, uint64_t shard_start,
                      uint64_t shard_end);
/* Same from host memory images of the three files (whole table; the shard is cut out here). */
int mic_db_load_host(mic_engine* e, const uint8_t* sizes, uint64_t htsize, const void* keys, int key_bytes,
                     const uint16_t* labels, uint32_t sampling, uint64_t shard_start, uint64_t shard_end);
/* Same from device memory images (d_keys/d_labels hold the WHOLE table's elements). */
int mic_db_load_device(mic_engine* e, const uint8_t* d_sizes, uint64_t htsize, const void* d_keys, int key_bytes,
                       const uint16_t* d_labels, uint32_t sampling, uint64_t shard_start, uint64_t shard_end);
/* Table-sharded runs (the reference's multi-device mode: m_partPointer ranges, CuClarkDB.cu:566-574, every device
 * queried with all reads :886-890, partial rows summed :934-1001).  Call BEFORE mic_db_load_* (whole table: shard_start
 * = shard_end = 0): the engine then answers for part `part` of `n_parts` of the database, and the per-read rows of the
 * n_parts engines sum to the whole table's (mic_merge_rows_device / mic_batch_merge_shards).  HOW the database is cut
 * follows the resident layout.  The super-k-mer layouts cut their resident table by SLOT range: a slot is chosen by
 * the minimizer, so all k-mers of a run of a read (one super-k-mer) belong to one part - a part loads and searches
 * 1/n_parts of the slots and the per-run kernel keeps its form (one compare per run).  The bucket cut of the on-disk
 * hash (c mod HTSIZE) would scatter the k-mers of one super-k-mer over all parts.  The other layouts keep the
 * reference's cut: part p answers for the buckets [HTSIZE p / n, HTSIZE (p + 1) / n).  Each part is built from the
 * whole .sz/.ky/.lb images (all parts size the table identically); n_parts <= 1 clears the setting.
 * shard_start / shard_end of mic_db_load_* remain the explicit bucket-range form (not combinable with a part). */
int mic_db_set_part(mic_engine* e, uint32_t part, uint32_t n_parts);
/* Device memory the caller is about to allocate on this engine's device WHILE the next mic_db_load_* runs (e.g. the ingest
 * slots, set up on a side thread): the table builders size their staging areas from the free HBM minus this, so the layout
 * and the number of build passes do not depend on which allocation comes first.  0 clears it. */
int mic_db_reserve_hbm(mic_engine* e, uint64_t bytes);
/* ---- several devices in one process (the command line's -d N; the reference: CuClarkDB ctor + read, CuClarkDB.cu:104-208, 461-808) ----
 * mic_peer_matrix       the reference checks and enables peer access for every pair of its devices before it merges their
 *                       partial rows with cudaMemcpyPeer (CuClarkDB.cu:184-208, 954-974).  Here: matrix[i * n + j] = 1 when device
 *                       i reaches device j's memory directly (hipDeviceCanAccessPeer; enabled once per ordered pair, "already
 *                       enabled" is fine), 0 when copies between the two are staged through host memory by the runtime; the
 *                       diagonal is 1.  n_devices <= mic_device_count.  The table-sharded exchange calls it for its engines itself.
 * mic_db_load_files_multi   the database of mic_db_load_files into n engines from ONE read of <prefix>.sz/.ky/.lb: every chunk
 *                       of the files is read once into pinned memory and uploaded to every device that hosts an engine; the
 *                       tables - each engine's part when mic_db_set_part was called, the whole table otherwise - are then built
 *                       by one thread per device at the same time.  Engines that share a device share its copy of the images. */
int mic_peer_matrix(int* matrix, int n_devices);
/* Free and total memory of a device in bytes (hipMemGetInfo): how many parts a table needs is decided from it. */
int mic_device_memory(int device, uint64_t* free_bytes, uint64_t* total_bytes);
int mic_db_load_files_multi(mic_engine* const* engines, size_t n_engines, const char* prefix, int key_bytes, uint32_t sampling);
/* Name of the query-kernel instantiation mic_query_device / the batch API / the ingest path launch for this engine's table (what
 * rocprofv3's kernel trace shows), e.g. "query_kernel_r<31, 20, false, true, false>"; returns the length, < 0 without a table. */
int mic_db_kernel_name(const mic_engine* e, char* buf, size_t cap);
int mic_db_get_info(const mic_engine* e, mic_db_info* info);
int mic_db_unload(mic_engine* e);
/* Stage times of the last table build of this process, one "<stage>: <seconds>" per line (what MIC_LOAD_TIMING=1 prints on
 * stderr); valid until the calling thread asks again.  The reference prints its load time, CuCLARK_hh.hh:610-625. */
const char* mic_db_last_build_report(void);

/* ---- batch API: the calls CuCLARK_hh.hh makes on CuClarkDB ----------------------------------
 * mic_batches_alloc   = CuClarkDB::malloc        (CuClarkDB.cu:317-419;  caller CuCLARK_hh.hh:1600-1606)
 *   The engine allocates pinned host buffers and lends them out; the caller fills
 *   reads_pointer[b] / containers[b] for batch b and reads results after mic_batch_wait.
 *   index_batches[num_batches+1] = index of the first read of each batch; results/rows are indexed
 *   by global read index.  rows is NULL unless extended != 0.
 * mic_batch_ready     = CuClarkDB::readyBatch    (CuClarkDB.cu:864-873;  caller :1735)
 * mic_batch_query     = CuClarkDB::queryBatch    (CuClarkDB.cu:878-1033; caller :1743,:1772)
 *   H2D, fused query kernel, result, D2H, event — asynchronous.  `followup` (swap cycles) is accepted
 *   and ignored: the whole table is resident, there are no cycles.
 * mic_batch_wait      = CuClarkDB::waitForBatch  (CuClarkDB.cu:440-445;  caller :1997,:2006)
 * mic_batch_check     = CuClarkDB::checkBatch    (CuClarkDB.cu:450-456)  *done = 1 when finished
 * mic_sync            = CuClarkDB::sync          (CuClarkDB.cu:424-435)
 * mic_batches_free    = CuClarkDB::freeBatchMemory (CuClarkDB.cu:279-312)
 * Threading: distinct batches may be filled concurrently; mic_batch_query is internally serialised;
 * mic_batch_wait may be called from another thread (reference: CuCLARK_hh.hh:1738-1760). */
int mic_batches_alloc(mic_engine* e, size_t num_reads_total, size_t max_reads, size_t max_containers,
                      const uint32_t* index_batches, int extended, uint32_t** results, uint32_t** rows,
                      uint32_t** reads_pointer /*[num_batches]*/, uint16_t** containers /*[num_batches]*/);
int mic_batch_ready(mic_engine* e, size_t batch, size_t n_reads, size_t n_containers);
int mic_batch_query(mic_engine* e, size_t batch, int extended, int followup);
int mic_batch_wait(mic_engine* e, size_t batch);
/* Dense per-target counts (u32[num_targets]) of read `read_in_batch` of a finished batch whose sparse row did
 * not fit (row[0] == MIC_ROW_INVALID); the reference has no equivalent — it truncates at MAXHITS and corrupts
 * the row (CuClarkDB.cu:1200-1211).  Synchronous; valid until the batch is queried again or freed. */
int mic_batch_dense_counts(mic_engine* e, size_t batch, size_t read_in_batch, uint32_t* counts);
int mic_batch_check(mic_engine* e, size_t batch, int* done);
/* Table-sharded batches: the reference's multi-device mode (CuClarkDB.cu:934-1001 - queryBatch on every device, the
 * partial result rows copied to device 0 with cudaMemcpyPeer, summed by mergeKernel, finished by resultKernel).
 * Every engine holds one bucket range of the same database (mic_db_load_*: shard_start, shard_end), the same batch
 * geometry (mic_batches_alloc with extended = 1) and was given the same packed reads for `batch`
 * (mic_batch_ready + mic_batch_query(extended = 1) on each).  The call waits for all of them, sums the sparse rows
 * into engines[0] and leaves best / second-best and the merged rows in engines[0]'s host arrays.  A read whose merged
 * row does not fit (MIC_FLAG_ROW_OVERFLOW in its results word 6, row[0] == MIC_ROW_INVALID) is completed by the
 * caller: the sum over the engines of mic_batch_dense_counts.  Synchronous.  Engines may share a device. */
int mic_batch_merge_shards(mic_engine* const* engines, size_t n_engines, size_t batch);
/* queryBatch on every engine of a table-sharded group from ONE upload (the reference copies the batch's host arrays to every device,
 * CuClarkDB.cu:886-890): the reads are engines[0]'s (filled into ITS lent buffers, mic_batch_ready on engines[0]); engines[0]
 * uploads them, the other engines take the packed reads from engines[0]'s device buffers by peer copy on their batch's stream and
 * run their kernel; all asynchronous, as mic_batch_query.  Follow with mic_batch_merge_shards.  The other engines' host buffers
 * for this batch are not read. */
int mic_batch_query_group(mic_engine* const* engines, size_t n_engines, size_t batch, int extended);
/* (How the rows are summed: READ-RANGE OWNED, all engines at once - engine j fetches the rows of the j-th 1/n of the batch's
 * reads from the other n - 1 engines (n - 1 peer copies of 1/n of the rows each, hipMemcpyPeerAsync over xGMI with peer access
 * enabled), sums them, finishes best / second-best for its range and writes results and rows of the range straight into
 * engines[0]'s host arrays.  The reference funnels whole row arrays into device 0 one after another, CuClarkDB.cu:954-974.
 * Peer copies, not RCCL: one process drives all devices here, the copy engines move the rows while the compute units run the
 * next batch's kernels, and there is nothing to rendez-vous; the one-process-per-GPU form of the same exchange is bench.py's
 * all_to_all over RCCL, cuclark_amd/multi.py.) */
int mic_sync(mic_engine* e);
/* Host threads that fill the engine's pinned buffers should run on the socket the device hangs off: on != 0 binds the
 * calling thread to the CPUs of the device's NUMA node, on == 0 restores its previous mask (no-op when the node is
 * unknown or MIC_NO_NUMA is set).  The engine's own pinned allocations are made there already. */
int mic_thread_bind_near_device(mic_engine* e, int on);
int mic_batches_free(mic_engine* e);

/* ---- device-resident entry points (kernels only; inputs/outputs already in HBM) --------------
 * mic_query_device: queryKernel + resultKernel fused (CuClarkDB.cu:1045-1243,1421-1471).
 *   d_results: n_reads*MIC_RESULT_WORDS u32.  d_rows: n_reads*row_words u32 or NULL.
 *   Reads whose register row (64 distinct targets) or sparse row overflowed are flagged and listed in an
 *   engine-owned device list; mic_resolve_flagged_device completes them exactly with the dense path.
 *   d_containers must be 4-byte aligned and readable for 32 elements past the last container (the kernel prefetches
 *   windows as aligned dwords); MIC_E_INVALID otherwise.
 *   stream: a hipStream_t (NULL = the engine's stream).  Asynchronous. */
int mic_query_device(mic_engine* e, const uint32_t* d_reads_pointer, const uint16_t* d_containers, size_t n_reads,
                     uint32_t* d_results, uint32_t* d_rows, void* stream);
/* Completes the reads flagged by the LAST mic_query_device call (same buffers, same stream): waits for the
 * stream, runs the dense kernels for the listed reads and patches d_results / d_rows.  *n_resolved
 * (optional) receives how many reads took the dense path.  Synchronous. */
int mic_resolve_flagged_device(mic_engine* e, const uint32_t* d_reads_pointer, const uint16_t* d_containers,
                               uint32_t* d_results, uint32_t* d_rows, void* stream, size_t* n_resolved);
/* mergeKernel (CuClarkDB.cu:1321-1415): out = a (+) b per read (sum by target); rows as above. */
int mic_merge_rows_device(mic_engine* e, const uint32_t* d_rows_a, const uint32_t* d_rows_b, uint32_t* d_rows_out,
                          size_t n_reads, void* stream);
/* resultKernel (CuClarkDB.cu:1421-1471) on sparse rows. */
int mic_result_from_rows_device(mic_engine* e, const uint32_t* d_rows, uint32_t* d_results, size_t n_reads,
                                void* stream);
/* Dense per-read per-target counts (u32 [n_reads*num_targets]) for the listed reads: the exact
 * fallback for reads whose rows overflow, and the --extended source of truth. */
int mic_count_dense_device(mic_engine* e, const uint32_t* d_reads_pointer, const uint16_t* d_containers,
                           const uint32_t* d_read_ids, size_t n_ids, uint32_t* d_counts, void* stream);
/* resultKernel on DENSE counts (u32 [n_ids * num_targets], e.g. mic_count_dense_device's, or their sum over the shards of
 * a table-sharded run): writes result row d_ids[i] (or i when d_ids is NULL) of d_results, and the sparse row when d_rows is
 * given and it fits.  This is how a read with more targets than a sparse row holds is completed exactly across shards. */
int mic_result_from_dense_device(mic_engine* e, const uint32_t* d_counts, const uint32_t* d_ids, size_t n_ids,
                                 uint32_t* d_results, uint32_t* d_rows, void* stream);
/* Bookkeeping for the roofline figure (not timed): out = {k-mers in the reads, k-mers whose bucket lies in this
 * engine's shard, hits, sum of the lengths of the probed buckets}.  Synchronous. */
int mic_probe_stats_device(mic_engine* e, const uint32_t* d_reads_pointer, const uint16_t* d_containers, size_t n_reads,
                           uint64_t out[4]);
/* Duration in ms of the last mic_query_device launch on this engine, measured with HIP events on the
 * stream it ran on (blocks until it finished). */
int mic_last_query_ms(mic_engine* e, float* ms);
/* Bookkeeping of the last mic_query_device launch on a super-k-mer table with a side table of crowded minimizers
 * (microsatellites; see mic_db_info.side_kmers): out = {reads that met a crowded minimizer and were finished by the
 * follow-up kernel, crowded runs handed to it, words of spilled rows, reads sent to the dense path for lack of room in
 * the work area}.  All zero for any other table.  Synchronous. */
int mic_last_crowd_stats(mic_engine* e, uint32_t out[4]);
/* test hook: the first `words` 32-bit words of the work area of the last mic_query_device launch (mic_internal.h: header, pending reads,
 * items, pool) and its capacities {pending reads, items, pool words}; MIC_E_STATE when the engine has none.  Synchronous. */
int mic_debug_fetch_crowd(mic_engine* e, uint32_t* out, size_t words, uint32_t caps[3]);
/* test hook: slots [first, first + n) of a whole (not parted) super-k-mer table, main slots first, then the continuation slots, as the
 * kernels read them: 32 words each - sort keys 0..5, three region words per entry 6..23, presence mask << 16 | label 24..29, entries
 * here | 0x100 if a continuation slot follows in word 30, its index in word 31.  n <= mic_db_info.n_slots - first.  Synchronous. */
int mic_debug_fetch_slots(mic_engine* e, uint64_t first, uint64_t n, uint32_t* out);

/* ---- device-side ingest: raw FASTA / FASTQ bytes in, result-CSV text out ----------------------------------------
 * The reference does the read indexing (CuCLARK_hh.hh:1339-1534), the 2-bit packing with its N-splitting
 * (CuCLARK_hh.hh:1616-1716) and the CSV lines (printExtendedResultsSynced, CuCLARK_hh.hh:1951-2139) on host threads
 * around queryBatch; at MI355X kernel rates those loops are the bottleneck by two orders of magnitude.  Here a batch
 * of WHOLE records is handed over as the bytes of the file and comes back as the bytes of the CSV (no header line,
 * non-extended format): line index, record index, packer, query kernel and CSV formatter all run on the device,
 * the host only moves bytes.  Output is byte-identical to mic_index_reads + mic_pack_reads + mic_batch_query +
 * mic_csv_line on the same bytes.
 *
 * mic_ingest_alloc    engine-owned pinned input buffers (raw[i], max_bytes each, 4 KiB .. 128 MiB) lent to the caller, as
 *                     CuClarkDB::malloc lends its batch buffers (CuClarkDB.cu:355-360); target_names as in mic_csv_line.
 * mic_ingest_classify blocking; slot-private stream: call it from one host thread per slot to keep the device busy.
 *                     The slot's first byte must be '>' (FASTA, also the merged paired-end text of file.cc:205-268 with
 *                     MIC_INGEST_PAIRED in flags) or '@' (FASTQ; with MIC_INGEST_FASTQ_2LINE two lines per record).
 *                     out->status == MIC_INGEST_OK: out->csv / csv_bytes / n_reads are valid until the slot's next call.
 *                     out->status & MIC_INGEST_FALLBACK: the batch holds something the device path does not
 *                     reproduce (the other bits say what); nothing was produced and the caller runs the host path
 *                     (mic_index_reads ... mic_csv_line) on these bytes.
 * mic_ingest_fetch_packed  test hook: the packed reads of the slot's last batch as the query kernel saw them. */
#define MIC_INGEST_PAIRED 1        /* flags: objects are merged pairs: Length column minus the separator (CuCLARK_hh.hh:2119)        */
#define MIC_INGEST_FASTQ_2LINE 2   /* flags: FASTQ records come as header + sequence line only (the caller dropped the '+' and
                                      quality lines, which nothing reads: halves the bytes that cross the host link)           */
#define MIC_INGEST_RESIDENT 4       /* flags: the slot's DEVICE buffer already holds the n_bytes of FASTA text - merged pairs
                                      (mic_pairs_merge_to_slot, with MIC_INGEST_PAIRED) or records of a FASTA text
                                      (mic_text_to_slot): nothing is uploaded                                                    */
#define MIC_INGEST_RESIDENT_FASTQ 12 /* flags: as MIC_INGEST_RESIDENT, and the text is four-line FASTQ (mic_text_to_slot), not merged pairs */
#define MIC_INGEST_NO_CSV 16       /* flags: no CSV (summary-only runs: mic_abundance_*): the CSV kernels and the copy of the text are
                                      skipped, csv_bytes is 0; results still come back with want_results, the status bits that
                                      do not come from CSV line lengths are raised as without the flag                          */
#define MIC_INGEST_OK 0u
#define MIC_INGEST_FALLBACK 1u     /* run the host path on this batch                                        */
#define MIC_INGEST_ODD_RECORD 2u   /* empty read name, FASTA record without a sequence line, unknown format   */
#define MIC_INGEST_TRUNCATED 4u    /* FASTQ line count not a multiple of four                                 */
#define MIC_INGEST_LONG_READ 8u    /* a sequence of more than MIC_MAX_PART bytes                              */
#define MIC_INGEST_TOO_MANY 16u    /* more lines / reads / containers / CSV bytes than the slot was sized for */
#define MIC_INGEST_DENSE 32u       /* a read needs the dense fallback (more than 64 targets hit)              */

typedef struct mic_ingest_result {
  uint64_t n_reads;
  uint64_t csv_bytes;
  const char* csv;           /* pinned host memory of the slot                                    */
  const uint32_t* results;   /* MIC_RESULT_WORDS per read when want_results was set, else NULL    */
  uint32_t status;
  uint32_t n_lines;
} mic_ingest_result;

int mic_ingest_alloc(mic_engine* e, size_t n_slots, size_t max_bytes, const char* const* target_names, uint32_t n_targets,
                     int want_results, uint8_t** raw /*[n_slots]*/);
int mic_ingest_classify(mic_engine* e, size_t slot, size_t n_bytes, int flags, mic_ingest_result* out);
/* The same for a table-sharded run (cuCLARK --db-sharded): group[p] holds part p of n_group parts of the database
 * (mic_db_set_part(p, n_group)); the slot belongs to group[owner] (mic_ingest_alloc on that engine), which indexes and packs the
 * batch and formats its CSV.  In between, every engine of the group probes ALL reads of the batch against its part (the packed
 * reads travel to the other engines by peer copy: 44 B per 150-bp read), and the per-read sparse rows are summed READ-RANGE
 * OWNED: engine j fetches the rows of the j-th 1/n_group of the reads from the other engines, sums, finishes best / second-best
 * and sends the 32-byte results of its range to the owner - all engines at once, nothing funnels through one device (the
 * reference: queryBatch on every device, cudaMemcpyPeer of whole row arrays into device 0, CuClarkDB.cu:886-1001).  A batch with
 * a read whose summed row does not fit (more than 15 targets) comes back as MIC_INGEST_FALLBACK | MIC_INGEST_DENSE like any other
 * batch the device path hands back.  n_group == 1 is mic_ingest_classify.  Blocking; one host thread per slot. */
int mic_ingest_classify_group(mic_engine* const* group, size_t n_group, size_t owner, size_t slot, size_t n_bytes, int flags,
                              mic_ingest_result* out);
int mic_ingest_fetch_packed(mic_engine* e, size_t slot, uint32_t* reads_pointer, size_t rp_cap, uint16_t* containers,
                            size_t cont_cap, uint64_t* n_reads, uint64_t* n_containers);
/* mic_ingest_fetch_group_rows  test hook: the partial sparse rows (row_words u32 per read) engine `part` of the slot's group
 * computed for the slot's last table-sharded batch, as its kernel wrote them. */
int mic_ingest_fetch_group_rows(mic_engine* owner, size_t slot, size_t part, uint32_t* rows, size_t cap_words, uint64_t* n_reads,
                                uint32_t* row_words);
/* mic_ingest_group_stats  what the table-sharded batches of this engine's slots cost, when the process runs with
 * MIC_GROUP_TIMING=1 (HIP events on every engine's stream; a measuring mode: the exchange then starts when ALL engines' rows are
 * written, so that its bracket holds copies and merges only).  out[0 .. MIC_GROUP_STATS_FIELDS): batches, reads, bytes of the
 * packed-read fan-out (owner -> the other engines), its ms summed over the helpers and over the batches, the same with the
 * slowest helper of each batch only, query-kernel ms summed over engines and batches, slowest engine of each batch only, bytes of
 * the row exchange (rows of a read range from the other engines + the results to the owner), its ms summed, slowest engine only.
 * Returns the number of fields (> 0: the one entry point that does not return MIC_OK on success) or a negative code; zeros
 * without MIC_GROUP_TIMING.  (The reference times nothing per device; its exchange is
 * CuClarkDB.cu:954-974.) */
#define MIC_GROUP_STATS_FIELDS 10
int mic_ingest_group_stats(mic_engine* owner, double* out, size_t cap);
int mic_ingest_free(mic_engine* e);
/* ---- base-quality mask: FASTQ bases below a Phred threshold take no part in any k-mer (csrc/mic_qmask.h: the rule) ---------
 * The reference reads no qualities (CuCLARK_hh.hh:1496-1523 steps over the quality line).  With a threshold byte c0 = offset + Q
 * (offset 33 or 64), byte i of a record's sequence line is MASKED iff the record's quality line has no byte i or that byte is below
 * c0 (unsigned compare; lines are taken without their '\n', a '\r' belongs to the line; surplus quality characters are ignored).
 * A masked byte is to the packer what an 'N' is: it ends the ACGTU run and belongs to no k-mer.  Length column, names, the
 * separator of a merged pair and gamma's denominator do not change: the result is that of the same text with every masked base
 * replaced by 'N', byte for byte.
 * mic_ingest_set_min_quality  engine state; 0 clears it, a value above 255 is MIC_E_INVALID.  From then on it applies to every
 *                             mic_ingest_classify / mic_ingest_classify_group call owned by this engine whose text is four-line
 *                             FASTQ (uploaded or MIC_INGEST_RESIDENT_FASTQ: masked in the packer), and to mic_pairs_merge_to_slot /
 *                             mic_pairs_text on this engine (each mate masked from its own quality line while it is merged).
 *                             MIC_INGEST_FASTQ_2LINE while a threshold is set: MIC_E_INVALID (the qualities are gone).  FASTA text
 *                             is unaffected.
 * mic_fastq_mask_quality      the rule on the CPU, no device needed: a copy of four-line FASTQ text with the masked bases replaced
 *                             by 'N' (in == out is allowed; threshold_byte 0: a plain copy).  MIC_E_INVALID when the text does not
 *                             start with '@' or its line count (an unterminated last line counts) is no multiple of four; nothing
 *                             is written then.  For what stays on the host: batches handed back (MIC_INGEST_FALLBACK), the batch path. */
int mic_ingest_set_min_quality(mic_engine* e, uint32_t threshold_byte);
int mic_fastq_mask_quality(const uint8_t* in, size_t nb, uint32_t threshold_byte, uint8_t* out);
/* ---- low-complexity mask: bases inside homopolymer / microsatellite sequence take no part in any k-mer (csrc/mic_lowc.h: the rule) --
 * CLARK databases are built from unmasked genomes, so a poly-A tail or an (AC)n tract of a read is probed like any other sequence; the
 * reference has no such mask.  A RUN is a maximal sequence of ACGTU bytes (either case) of a record's sequence - the packer's part
 * before its length test: '\n' is transparent (wrapped FASTA lines join), every other byte ends it ('\r', 'N', a base masked by the
 * base-quality mask: runs are taken after that mask).  With the run's n nucleotides x[0..n) in the packer's 2-bit code and triplets
 * t[j] = 16 x[j] + 4 x[j+1] + x[j+2], the WINDOW of base i is [lo, hi) = [max(0, i-16), min(n, i+16)): width 32, centred, clipped to
 * the run, never across an 'N', the joint of a merged pair or a record end.  l = hi - lo - 2 triplets t[lo .. lo+l) lie in it, c_v of
 * them have the value v, T = sum_v c_v (c_v - 1) / 2.  Base i is MASKED iff l >= 2 and 10 T > level (l - 1): DUST's score above
 * level / 10, on a fixed window of about k nucleotides - not symmetric DUST's perfect intervals, so another tool's report differs at
 * tract edges.  Level 20 is DUST's customary level.  A masked base is to the packer what an 'N' is; Length column, names and gamma's
 * denominator do not change: the result is that of the same text with every masked base replaced by 'N', byte for byte.  The rule is
 * not idempotent (what is left between two masked stretches is a new, shorter run): it is applied once, to the original text.
 * mic_ingest_set_low_complexity  engine state; 0 clears it, a level above 149 is MIC_E_INVALID (150 could mask nothing).  From then on
 *                                it applies to every mic_ingest_classify / mic_ingest_classify_group call owned by this engine: FASTA
 *                                (merged pairs included), four-line FASTQ and MIC_INGEST_FASTQ_2LINE text, uploaded or resident.  A
 *                                kernel in front of the packer writes one bit per text byte into a bitmap of the slot (allocated with
 *                                the slot's first such batch); the slot's text is not rewritten, so a resident text can be classified
 *                                again.  With the level 0 nothing is launched and nothing is allocated.
 * mic_text_mask_low_complexity   the rule on the CPU, no device needed: a copy of FASTA or four-line FASTQ text with the masked bases
 *                                replaced by 'N' (in == out is allowed; level 0: a plain copy); records are those of mic_index_reads.
 *                                Linear in the text.  MIC_E_INVALID, nothing written, when the text does not start with '>' or '@' or
 *                                the level is above 149.  For what stays on the host: batches handed back, the batch path. */
int mic_ingest_set_low_complexity(mic_engine* e, uint32_t level);
int mic_text_mask_low_complexity(const uint8_t* in, size_t nb, uint32_t level, uint8_t* out);
/* ---- compressed input: one gzip member inflated on the device ------------------------------------------------
 * Replaces the `gunzip` the reference's scripts run in front of the classifier (classify_metagenome.sh:116-142) for the
 * common cases: ONE member without a preset dictionary (what `gzip` writes), or a whole block-gzip file (BGZF: members with a
 * 'BC' size subfield, what bgzip / samtools write).  `gz` = the whole .gz file in host memory.  On MIC_OK *d_text is a
 * device buffer of *n_text bytes of text (mic_gz_free_text releases it, mic_gz_copy_text copies a piece to the host);
 * length (ISIZE) and CRC-32 of the member - of every member of a block-gzip file - have been checked against the trailer, as
 * gunzip checks them; *crc32_expected is the one member's CRC-32 (0 for block gzip).
 * MIC_E_UNSUPPORTED: several ordinary members, data behind the last block, or blocks that could not be found speculatively - the
 * caller inflates on the CPU (csrc/pgz.hpp / zlib) as before; MIC_E_INVALID: the data is damaged (zlib would fail too). */
int mic_gz_inflate_device(mic_engine* e, const void* gz, size_t gz_bytes, void** d_text, size_t* n_text, uint32_t* crc32_expected);
int mic_gz_copy_text(mic_engine* e, const void* d_text, size_t offset, size_t n, void* host_dst);
int mic_gz_free_text(mic_engine* e, void* d_text);
/* mic_gz_reserve: the device buffers of one mic_gz_inflate_device call for a file of gz_bytes bytes whose trailer says isize
 * (the last four bytes of the file), set up ahead of it - a fresh gigabyte of device memory takes the driver as long as the decode
 * does; the command line reserves while its database loads, as it does with its ingest slots (CuClarkDB::malloc's place in the
 * reference: CuCLARK_hh.hh:1600-1606).  The next call for a file of exactly this size uses them; mic_gz_release (also part of
 * mic_destroy) frees what the engine's reservations still hold.  mic_gz_reserve_bytes: what a reservation takes, for
 * mic_db_reserve_hbm. */
int mic_gz_reserve(mic_engine* e, size_t gz_bytes, uint32_t isize);
uint64_t mic_gz_reserve_bytes(size_t gz_bytes, uint32_t isize);
int mic_gz_release(mic_engine* e);
/* One plain member in STRIPES (round 6; BASELINE config 5, "gzip FASTQ ingest overlapped"): the units of the member - one per deflate
 * block - go through decode, stitching, windows and resolve a stripe of consecutive units at a time, and when a stripe is done its
 * text is final: the caller indexes and classifies it (mic_text_index_front_device, mic_text_to_slot) while the next stripe decodes.
 * mic_gz_stream_open   uploads the file, finds its blocks, hands out the text buffer of *n_text bytes (the trailer's ISIZE), nothing
 *                      of it final yet; `stripes` = how many pieces to cut the units into (>= 1).  Block gzip: MIC_E_UNSUPPORTED
 *                      (mic_gz_inflate_device takes it whole).
 * mic_gz_stream_next   the next stripe, synchronously: on MIC_OK the first *n_final bytes of the text are final; *done = 1 with the last
 *                      stripe, after length and CRC-32 were checked against the trailer.  MIC_E_UNSUPPORTED / MIC_E_INVALID as for
 *                      mic_gz_inflate_device - but possibly after text was handed out: a caller that used it starts over on its CPU
 *                      inflater (exe/cuCLARK does, classifier.cpp).
 * mic_gz_stream_close  frees everything; keep_text != 0: but the text, the caller's from then on (mic_gz_free_text). */
typedef struct mic_gz_stream mic_gz_stream;
int mic_gz_stream_open(mic_engine* e, const void* gz, size_t gz_bytes, uint32_t stripes, mic_gz_stream** out, void** d_text, size_t* n_text);
int mic_gz_stream_next(mic_gz_stream* s, size_t* n_final, int* done);
int mic_gz_stream_close(mic_gz_stream* s, int keep_text);

/* ---- paired-end FASTQ texts that are on the device already (inflated there): the reference's merge, on the device ----
 * file.cc:205-268 (mergePairedFiles) writes ">id\nseq1Nseq2\n" per pair of records, id = the header's first field between
 * the separators ' ', '/', '\t', '@' (file.cc:224), both ids equal.  The command line's loaders do that on the host for
 * files (classifier.cpp: PairedFileFeeder); for two texts in device memory (mic_gz_inflate_device of both mates):
 * mic_pairs_index_device  line index of both texts, every pair of records checked, the offsets of the merged records.
 *                         *status != 0 (MIC_PAIRS_*): these files are not what the line arithmetic covers - line counts that
 *                         differ or are no multiple of four, a header line without '@', ids that differ or are empty, a text
 *                         of 4 GiB or more; nothing is returned and the caller runs its host reader, which treats such
 *                         input the way the reference does.  The texts must stay allocated while the handle lives
 *                         (16 readable bytes behind each: mic_gz_inflate_device's buffers have them).
 * mic_pairs_offsets       host array: bytes of merged text in front of record i * stride (last entry: in front of record
 *                         n_records = the whole text), from which the caller cuts batches that fit its slots.
 * mic_pairs_merge_to_slot the merged text of records [r0, r1) written into an ingest slot's device buffer on the slot's
 *                         stream (r0 and r1 multiples of the stride, or n_records); then mic_ingest_classify(slot, *n_bytes,
 *                         MIC_INGEST_PAIRED | MIC_INGEST_RESIDENT).
 * mic_pairs_text          the same text copied to the host (for a batch the device path hands back).                  */
#define MIC_PAIRS_LINES 1u     /* line counts differ, are zero or no multiple of four */
#define MIC_PAIRS_HEADER 2u    /* a record whose first line is empty or has no '@' in front */
#define MIC_PAIRS_ID 4u        /* ids of a pair differ, or are empty */
#define MIC_PAIRS_BIG 8u       /* a text of 4 GiB or more (32-bit line starts), or an empty one */
typedef struct mic_pairs mic_pairs;
int mic_pairs_index_device(mic_engine* e, const void* d_text1, size_t n1, const void* d_text2, size_t n2, mic_pairs** out,
                           uint64_t* n_records, uint32_t* status);
int mic_pairs_offsets(const mic_pairs* p, const uint64_t** samples, size_t* n_samples, uint32_t* stride);
int mic_pairs_merge_to_slot(mic_engine* e, mic_pairs* p, uint64_t r0, uint64_t r1, size_t slot, size_t* n_bytes);
int mic_pairs_text(mic_engine* e, mic_pairs* p, uint64_t r0, uint64_t r1, void* host_dst, size_t cap, size_t* n_bytes);
int mic_pairs_free(mic_engine* e, mic_pairs* p);

/* ---- one FASTQ text that is on the device already (the inflated file of -O reads.fq.gz) ------------------------------------
 * mic_text_index_device  where the records start: FASTQ (the text begins with '@' and has a multiple of four lines) or FASTA (it
 *                        begins with '>'; a record is a '>' line and the lines up to the next one); else *status
 *                        (MIC_PAIRS_HEADER: something else, MIC_PAIRS_LINES, MIC_PAIRS_BIG) and the caller's host reader.
 * mic_text_format        '@' or '>': what the index found.
 * mic_text_offsets       host array: byte offset of record i * stride (last entry: the size of the text).
 * mic_text_to_slot       records [r0, r1) copied device to device into an ingest slot's buffer on the slot's stream; then
 *                        mic_ingest_classify(slot, *n_bytes, MIC_INGEST_RESIDENT_FASTQ, or MIC_INGEST_RESIDENT for FASTA): records the device path does not
 *                        reproduce come back as MIC_INGEST_FALLBACK as always, and mic_text_copy gives their bytes to the host. */
typedef struct mic_text mic_text;
int mic_text_index_device(mic_engine* e, const void* d_text, size_t n, mic_text** out, uint64_t* n_records, uint32_t* status);
/* the FRONT of a FASTQ text that is still growing (mic_gz_stream_next): its whole records - lines that end in a newline, four to a
 * record - are indexed, *n_used = where the first record that is not whole begins (the next call's text starts there).  No whole
 * record yet: MIC_OK, *out = NULL, *n_used = 0.  *status = MIC_PAIRS_HEADER when the text does not begin with '@'.  The rest of the
 * text, once it is all there: mic_text_index_device from where the last front ended (d_text need not be aligned for either). */
int mic_text_index_front_device(mic_engine* e, const void* d_text, size_t n, mic_text** out, uint64_t* n_records, uint64_t* n_used, uint32_t* status);
int mic_text_format(const mic_text* p);
int mic_text_offsets(const mic_text* p, const uint64_t** samples, size_t* n_samples, uint32_t* stride);
int mic_text_to_slot(mic_engine* e, mic_text* p, uint64_t r0, uint64_t r1, size_t slot, size_t* n_bytes);
int mic_text_copy(mic_engine* e, mic_text* p, uint64_t r0, uint64_t r1, void* host_dst, size_t cap, size_t* n_bytes);
int mic_text_free(mic_engine* e, mic_text* p);

/* ---- abundance profile: reads per target, counted on the device (CLARK's estimate_abundance step) ----------------------
 * A read's result row goes into one of num_targets + 2 u64 counters (csrc/mic_abund.h: the rule, shared by host and device):
 *   [0] unassigned (idxBest == 0), [1] assigned but filtered out, [idxBest + 1] the read counts for target idxBest - 1.
 * The filter: confidence best / (best + second) >= conf_num / conf_den and gamma sum / (norm - k + 1) >= gamma_num / gamma_den
 * (gamma_num == 0: no gamma filter), exact integer arithmetic; denominators are 10^d, d <= 9, numerators <= denominators.
 * norm = the CSV's Length column (the read's length, minus 1 for a merged pair).
 * mic_abundance_start   zeroes and enables the engine's counters: from then on every ingest batch of this engine that returns
 *                       MIC_INGEST_OK (mic_ingest_classify, or mic_ingest_classify_group with this engine as the owner) adds its
 *                       reads on the device; a batch handed back (MIC_INGEST_FALLBACK) adds nothing - the caller counts it
 *                       (mic_abundance_host) where it classifies it.  The batch API (mic_batch_*) does not count.
 * mic_abundance_fetch   waits for the engine's device, then copies the counters (n = num_targets + 2 words) out.
 * mic_abundance_stop    disables counting (the counters keep their values).
 * mic_abundance_device  the same rule on caller-owned device memory: d_results (MIC_RESULT_WORDS u32 per read), d_norm (u32 per
 *                       read; NULL: only a filter without gamma), counts ADDED to d_counts (num_targets + 2 u64).  Asynchronous
 *                       on `stream` (NULL = the engine's stream).
 * mic_abundance_host    the rule on the CPU (no device needed): counts added to counts[n_targets + 2].
 * mic_abund_parse       a threshold as the command lines take it ("0.75": digits, one optional '.', at most 9 fractional digits,
 *                       value in [0, max_int]; no sign, exponent or blanks) into num / den; MIC_E_INVALID otherwise. */
typedef struct mic_abund_filter {
  uint64_t conf_num, conf_den;    /* minimum confidence conf_num / conf_den (CLARK's default 0.5 = 5 / 10)       */
  uint64_t gamma_num, gamma_den;  /* minimum gamma (CLARK's default 0 = 0 / 1: no gamma filter)                   */
} mic_abund_filter;
int mic_abundance_start(mic_engine* e, const mic_abund_filter* filter);
int mic_abundance_fetch(mic_engine* e, uint64_t* counts, size_t n);
int mic_abundance_stop(mic_engine* e);
int mic_abundance_device(mic_engine* e, const uint32_t* d_results, const uint32_t* d_norm, size_t n_reads, const mic_abund_filter* filter,
                         uint64_t* d_counts, void* stream);
int mic_abundance_host(const uint32_t* results, const uint32_t* norm, size_t n_reads, int k, uint32_t n_targets,
                       const mic_abund_filter* filter, uint64_t* counts);
int mic_abund_parse(const char* text, uint32_t max_int, uint64_t* num, uint64_t* den);

/* ---- rank roll-up: every read resolved at the lowest confident level of a lineage (csrc/mic_rollup.h: the rule) ---------------
 * A lineage has n_levels (1 .. MIC_ROLLUP_MAX_LEVELS) levels above the targets: group_of[(l - 1) * num_targets + t] is the group of
 * target t at level l; level 0 is the targets themselves.  Ids at every level are numbered by first appearance in ascending target
 * order, and level l is a coarsening of level l - 1 (mic_rollup_check; MIC_E_INVALID otherwise).  A read's per-target counts (its
 * sparse row, or dense counts when the row did not fit) are summed per group, best / second-best are taken at every level by
 * resultKernel's rule, and the read is assigned at the LOWEST level whose confidence best / (best + second) passes the filter (gamma
 * as for mic_abundance_*: the same at every level).
 *   roll-up row  MIC_ROLLUP_WORDS u32: {sum, idxBest, best, idxSecond, second, level, flags, nGroupsHit}: indices are group + 1 at
 *                `level` (0 = none); no level passes: level = MIC_ROLLUP_UNRESOLVED, words 1-4 and 7 are level 0's; sum == 0: all
 *                zero; the sparse row is MIC_ROW_INVALID: level = MIC_ROLLUP_PENDING, flags = MIC_FLAG_ROW_OVERFLOW, nothing is
 *                counted and mic_rollup_dense_device (or mic_rollup_host with dense counts) completes the read.
 *   levels       optional, (n_levels + 1) * 4 u32 per read: {idxBest, best, idxSecond, second} of every level, level 0 first: the
 *                read classified at each rank.
 *   counters     u64 [2 + T + G_1 + .. + G_L] (mic_rollup_layout): [0] no hit, [1] unresolved, [2 + off_l + g] reads assigned
 *                to group g of level l, off_0 = 0, off_l = T + G_1 + .. + G_(l-1).  Every counted read adds one to exactly one.
 * mic_rollup_check         host only: MIC_OK or MIC_E_INVALID (mic_last_error names the level and the target).
 * mic_rollup_set           checks and installs a lineage on the engine (n_levels == 0 clears it); not while roll-up is started.
 * mic_rollup_layout        n_groups[0 .. n_levels] (n_groups[0] = num_targets) and the number of counters; either may be NULL.
 *                          Returns the number of levels (>= 1) or a negative code.
 * mic_rollup_device        sparse rows (the engine's row_words u32 per read) -> roll-up rows, optional levels, counters ADDED to
 *                          d_counts (optional).  d_norm as for mic_abundance_device.  Asynchronous on `stream`.
 * mic_rollup_dense_device  the same from dense counts (u32 [n_ids * num_targets], mic_count_dense_device's): writes roll-up row
 *                          and levels d_ids[i] (i when d_ids is NULL), flags = MIC_FLAG_DENSE_PATH; d_norm is indexed like them.
 * mic_rollup_host          the rule on the CPU, no device needed.  rows: row_words u32 per read; dense (optional): num_targets u32
 *                          per read, used for the reads whose row is MIC_ROW_INVALID (rows == NULL: for every read); without it
 *                          such reads come back MIC_ROLLUP_PENDING and uncounted.  rollup / levels / counts are optional.
 * mic_rollup_start / _fetch / _stop   the engine's counters over ingest batches, by the contract of mic_abundance_start / _fetch /
 *                          _stop: every batch that returns MIC_INGEST_OK adds its reads on the device, a batch handed back adds
 *                          nothing.  While started, a batch with a read whose row does not fit is handed back with
 *                          MIC_INGEST_DENSE.  mic_ingest_rollup_rows: the roll-up rows of the slot's last MIC_INGEST_OK batch
 *                          (pinned host memory, valid until the slot's next call) when the slots were allocated with want_results. */
#define MIC_ROLLUP_WORDS 8
#define MIC_ROLLUP_MAX_LEVELS 7
#define MIC_ROLLUP_UNRESOLVED 0xFFFFFFFFu
#define MIC_ROLLUP_PENDING 0xFFFFFFFEu
int mic_rollup_check(uint32_t n_targets, uint32_t n_levels, const uint16_t* group_of);
int mic_rollup_set(mic_engine* e, uint32_t n_levels, const uint16_t* group_of);
int mic_rollup_layout(const mic_engine* e, uint32_t* n_groups, uint64_t* n_counters);
int mic_rollup_device(mic_engine* e, const uint32_t* d_rows, const uint32_t* d_norm, size_t n_reads, const mic_abund_filter* filter,
                      uint32_t* d_rollup, uint32_t* d_levels, uint64_t* d_counts, void* stream);
int mic_rollup_dense_device(mic_engine* e, const uint32_t* d_dense, const uint32_t* d_ids, size_t n_ids, const uint32_t* d_norm,
                            const mic_abund_filter* filter, uint32_t* d_rollup, uint32_t* d_levels, uint64_t* d_counts, void* stream);
int mic_rollup_host(const uint32_t* rows, uint32_t row_words, const uint32_t* dense, const uint32_t* norm, size_t n_reads, int k,
                    uint32_t n_targets, uint32_t n_levels, const uint16_t* group_of, const mic_abund_filter* filter,
                    uint32_t* rollup, uint32_t* levels, uint64_t* counts);
int mic_rollup_start(mic_engine* e, const mic_abund_filter* filter);
int mic_rollup_fetch(mic_engine* e, uint64_t* counts, size_t n);
int mic_rollup_stop(mic_engine* e);
int mic_ingest_rollup_rows(mic_engine* e, size_t slot, const uint32_t** rollup, uint64_t* n_reads);

/* ---- score densities: assignments per confidence and per gamma score, counted on the device (CLARK's evaluate_density steps) ----
 * A read's result row goes into one cell of a 51 x 101 table of bins 0.01 wide (csrc/mic_density.h: the rule, shared by host and
 * device, exact integer arithmetic): confidence bin c = floor(100 best / (best + second)) in 50 .. 100, gamma bin
 * g = min(100, floor(100 sum / (norm - k + 1))) in 0 .. 100 (norm - k + 1 <= 0: g = 0); norm as for the abundance profile.
 *   counters  MIC_DENSITY_WORDS u64: [0] reads seen, [1] unassigned (idxBest == 0 or past the targets), [2 + (c - 50) * 101 + g].
 * The sum of the cells with c >= 100 conf and g >= 100 gamma is the number of reads the abundance filter {conf, gamma} keeps, for
 * thresholds of at most two decimals.
 * mic_density_start / _fetch / _stop   the engine's counters over ingest batches, by the contract of mic_abundance_start / _fetch /
 *                      _stop (n = MIC_DENSITY_WORDS): a batch that returns MIC_INGEST_OK adds its reads on the device, a batch handed
 *                      back adds nothing and the caller counts it with mic_density_host.  Freed with the engine.
 * mic_density_device   the rule on caller-owned device memory: d_results (MIC_RESULT_WORDS u32 per read), d_norm (u32 per read;
 *                      NULL: every read in gamma bin 0), counts ADDED to d_counts (MIC_DENSITY_WORDS u64).  At most 2^32 - 1 reads
 *                      per call.  Asynchronous on `stream` (NULL = the engine's stream).
 * mic_density_host     the rule on the CPU (no device needed): counts added to counts[MIC_DENSITY_WORDS].
 * mic_density_format   the report of exe/cuCLARK --density and exe/evaluate_density (csrc/density_report.hpp) as text: which = 0 all
 *                      four blocks, 1 the totals and the confidence block, 2 the totals and the gamma block.  Returns the length of the
 *                      text (written with a terminator when it fits cap; buf may be NULL to ask for the length) or MIC_E_INVALID. */
#define MIC_DENSITY_WORDS 5153
int mic_density_start(mic_engine* e);
int mic_density_fetch(mic_engine* e, uint64_t* counts, size_t n);
int mic_density_stop(mic_engine* e);
int mic_density_device(mic_engine* e, const uint32_t* d_results, const uint32_t* d_norm, size_t n_reads, uint64_t* d_counts, void* stream);
int mic_density_host(const uint32_t* results, const uint32_t* norm, size_t n_reads, int k, uint32_t n_targets, uint64_t* counts);
long mic_density_format(const uint64_t* counts, size_t n, int which, char* buf, size_t cap);

/* ---- k-mer sketches: distinct k-mers hit per target, sketched on the device (csrc/mic_ksketch.h: the rule, shared by host and device) ----
 * For every k-mer occurrence of every read whose table label is target t (what the query counts: per read part, none across an 'N',
 * masked bases included) the canonical k-mer goes into t's HyperLogLog sketch and t's hit counter grows by one:
 *   regs   u8[num_targets * MIC_KSKETCH_REGS]: register idx of target t (0-based) at regs[t * MIC_KSKETCH_REGS + idx]
 *   hits   u64[num_targets]
 * Registers merge by element-wise max and hits by sum: batches, engines and calls combine in any order with the same result.  The
 * rule does not depend on a confidence or gamma filter.
 * mic_ksketch_device    the rule on caller-owned device memory: packed reads as for mic_query_device, d_results the reads' result rows
 *                       (MIC_RESULT_WORDS u32 per read: a read whose sum is 0 is skipped), registers MAXED into d_regs and hits ADDED
 *                       into d_hits.  Only the k-mers this engine answers for count, so the sum over the engines of a sharded or parted
 *                       table is the whole table's.  Asynchronous on `stream` (NULL = the engine's stream).
 * mic_ksketch_start / _fetch / _stop   the engine's sketches (num_targets * 16 KiB + 8 B on its device, allocated and zeroed at
 *                       start, freed with the engine) over ingest batches, by the contract of mic_abundance_start / _fetch / _stop:
 *                       a mic_ingest_classify batch that returns MIC_INGEST_OK is added behind the query on the slot's stream, with
 *                       or without MIC_INGEST_NO_CSV; a batch handed back adds nothing (the caller classifies it through the batch
 *                       API and adds it with mic_batch_ksketch).  While started, mic_ingest_classify_group with more than one engine
 *                       returns MIC_E_UNSUPPORTED.  _fetch: n_regs = num_targets * MIC_KSKETCH_REGS, n_hits = num_targets.
 * mic_batch_ksketch     adds the reads of a batch of the batch API (after mic_batch_wait; its packed reads and results are still on
 *                       the device) to the engine's sketches.  MIC_E_STATE when they are not started.  Synchronous.
 * mic_ksketch_add_host  the rule on the CPU (no device needed) on n pairs (k-mer as it reads, label): label 0 or above n_targets
 *                       adds nothing, label l adds to target l - 1.
 * mic_ksketch_estimate  the number of distinct k-mers behind one target's MIC_KSKETCH_REGS registers (Ertl's improved raw estimator);
 *                       all registers zero: 0.  A negative value when regs is NULL.
 * mic_ksketch_format    the report of exe/cuCLARK --kmer-report (csrc/kmer_report.hpp) as text: names (n_targets strings), reads per
 *                       target (n_targets u64: what mic_abundance_* counts for it), the sketches.  Returns the length of the text
 *                       (written with a terminator when it fits cap; buf may be NULL to ask for the length) or MIC_E_INVALID. */
#define MIC_KSKETCH_REGS 16384
int mic_ksketch_device(mic_engine* e, const uint32_t* d_reads_pointer, const uint16_t* d_containers, size_t n_reads, const uint32_t* d_results,
                       uint8_t* d_regs, uint64_t* d_hits, void* stream);
int mic_ksketch_start(mic_engine* e);
int mic_ksketch_fetch(mic_engine* e, uint8_t* regs, size_t n_regs, uint64_t* hits, size_t n_hits);
int mic_ksketch_stop(mic_engine* e);
int mic_batch_ksketch(mic_engine* e, size_t batch);
int mic_ksketch_add_host(const uint64_t* kmers, const uint32_t* labels, size_t n, int k, uint32_t n_targets, uint8_t* regs, uint64_t* hits);
double mic_ksketch_estimate(const uint8_t* regs_of_one_target);
long mic_ksketch_format(const char* const* names, const uint64_t* reads, const uint8_t* regs, const uint64_t* hits, uint32_t n_targets,
                        char* buf, size_t cap);

/* ---- table census: the database's own k-mers probed through the resident table, counted per target (csrc/mic_census.h: the rule) ----
 * mic_db_get_info has totals only; the census says how many k-mers of EACH target the resident table holds - the denominator of the
 * coverage of exe/cuCLARK --kmer-coverage (distinct k-mers the reads touched / the target's k-mers in the table) - and checks the
 * table while it counts.  The elements are those the table builders enumerate from the .sz / .ky / .lb images (kept buckets under
 * `sampling`, entries the reference's scan reaches, c = key * htsize + bucket).  For each of them, with l = the lookup of a read that
 * is exactly this k-mer (position 0) and `mine` = this engine answers for it:
 *   stats[2]  c is not canonical (malformed databases only): nothing else happens
 *   stats[1]  !mine: another part (mic_db_set_part) or shard answers for it
 *   stats[0]  l == file label + 1; then counts[l - 1] += 1 when l <= num_targets, else stats[4] += 1 (in no counts entry)
 *   stats[3]  lost: not found, or found under another label
 * counts is u64[num_targets], stats u64[8] (stats[5 .. 7] are 0).  A healthy whole table shows stats[3] == 0, stats[0] ==
 * mic_db_info.n_elems (a well-formed database) and sum(counts) == stats[0] - stats[4]; the parts' counts sum to the whole table's.
 * mic_db_census_enable  before mic_db_load_*: the load then ends with the census (one kernel behind the build, while the images are
 *                       still on the device; num_targets * 8 + 64 bytes of device memory until mic_db_unload; a "census: <seconds>"
 *                       line in mic_db_last_build_report).  stats[3] != 0 fails the load with MIC_E_INVALID ("table census: N k-mers
 *                       are not found under their label").  MIC_E_STATE once a table is loaded.  Off (the default): nothing is
 *                       allocated or launched.
 * mic_db_census_fetch   the loaded table's census from host copies; n == num_targets.  MIC_E_STATE when the table was loaded without
 *                       mic_db_census_enable.
 * mic_db_census_device  the rule on caller-owned device images (whole: d_sizes[htsize], the keys and labels of every bucket; the loaded
 *                       table's htsize and key_bytes) over the buckets [s0, s1) (s1 == 0: htsize) against the loaded table; ADDS to
 *                       d_counts (u64[num_targets]) and d_stats (u64[8]).  Runs on `stream` (NULL = the engine's) and waits for it.
 * mic_db_census_host    the rule on the CPU (no device needed): the enumeration and the canonical test; there is no table to probe, so
 *                       every canonical element counts under its file label - what a healthy whole table returns.  ADDS to counts
 *                       (u64[n_targets]) and stats (u64[8]).
 * mic_kcoverage_format  the report of exe/cuCLARK --kmer-coverage (csrc/kmer_report.hpp) as text: mic_ksketch_format's arguments and
 *                       target_kmers (n_targets u64: the census counts).  Returns the length of the text (written with a terminator
 *                       when it fits cap; buf may be NULL to ask for the length), or MIC_E_INVALID: a null argument, or a target with
 *                       hits and no k-mers in the table (no healthy table gives one). */
int mic_db_census_enable(mic_engine* e, int on);
int mic_db_census_fetch(const mic_engine* e, uint64_t* counts, size_t n, uint64_t stats[8]);
int mic_db_census_device(mic_engine* e, const uint8_t* d_sizes, uint64_t htsize, const void* d_keys, int key_bytes, const uint16_t* d_labels,
                         uint32_t sampling, uint64_t s0, uint64_t s1, uint64_t* d_counts, uint64_t* d_stats, void* stream);
int mic_db_census_host(const uint8_t* sizes, uint64_t htsize, const void* keys, int key_bytes, const uint16_t* labels, uint32_t sampling, int k,
                       uint32_t n_targets, uint64_t* counts, uint64_t stats[8]);
long mic_kcoverage_format(const char* const* names, const uint64_t* reads, const uint8_t* regs, const uint64_t* hits, const uint64_t* target_kmers,
                          uint32_t n_targets, char* buf, size_t cap);

/* ---- read splitting: the classified and the unclassified reads themselves, partitioned on the device (csrc/mic_split.h: the rule) ----
 * The reference says what every read is and cannot hand the reads back.  Record r of a text is the bytes from the first byte of its
 * header line up to the first byte of the next record's header line (the last record: to the end of the text); records are those of
 * the library's indexers and tile the text.  A record is CLASSIFIED iff it counts for a target under the abundance filter (bucket >= 2
 * of mic_abundance_*: norm and filter exactly as there), UNCLASSIFIED otherwise.  Each class's records are concatenated in input order,
 * byte for byte ('\r', wrapped lines, '+' and quality lines, trailing blank lines of the last record); a text whose last byte is not
 * '\n' gets one '\n' appended to its last record - the only byte ever added.  The masks (mic_ingest_set_min_quality /
 * _low_complexity) change which class a record falls into, never its bytes.
 *   partition buffer  nb + 1 bytes: classified records at [0, a), unclassified records at [a, a + b), a + b = nb or nb + 1.  A class
 *                     that `which` does not name is not copied: its part of the buffer is left as it was.
 *   totals            u64[4] = {a, b, classified records, unclassified records}
 * mic_split_start / _stop  engine state, next to mic_abundance_start: from then on every mic_ingest_classify / _group batch owned by
 *                        this engine that returns MIC_INGEST_OK is partitioned behind the query, on the slot's stream, and the text of
 *                        the classes asked for is brought to a pinned buffer of the slot (allocated, with its device twin, by
 *                        mic_ingest_alloc when the split is started by then, else with the slot's first such batch); with and without MIC_INGEST_NO_CSV; a batch handed back (MIC_INGEST_FALLBACK)
 *                        produces nothing and the caller splits it with mic_split_host.  MIC_INGEST_FASTQ_2LINE while started:
 *                        MIC_E_INVALID (the quality lines are gone).  In a table-sharded group the owner splits, from the group's final
 *                        results.  A filter that fails the test of mic_abundance_start: MIC_E_INVALID.
 * mic_ingest_split_text  the split of the slot's last batch: pointers into the slot's pinned buffer, valid until the slot's next call
 *                        (a class that was not asked for: NULL and 0 bytes; its record count is still given); MIC_E_STATE when the
 *                        slot's last batch left none.  Any out pointer may be NULL.
 * mic_split_device       the kernels alone on caller-owned device memory: d_text (nb bytes, 1 B .. 128 MiB, 4-byte aligned),
 *                        d_rec_start (u32 per record, ascending, [0] = 0), d_results, d_norm (NULL: only a filter without gamma),
 *                        d_out (nb + 1 bytes, 4-byte aligned).  Synchronous on `stream` (NULL = the engine's stream).
 * mic_split_host         the rule on the CPU, no device needed: rec_start as u64 (mic_index_reads: name_s - 1), `out` of nb + 1 bytes.
 *                        MIC_E_INVALID when the starts do not begin at 0, do not ascend or reach nb. */
#define MIC_SPLIT_CLASSIFIED 1
#define MIC_SPLIT_UNCLASSIFIED 2
int mic_split_start(mic_engine* e, const mic_abund_filter* filter, int which);
int mic_split_stop(mic_engine* e);
int mic_ingest_split_text(mic_engine* e, size_t slot, const uint8_t** classified, uint64_t* classified_bytes, uint64_t* n_classified,
                          const uint8_t** unclassified, uint64_t* unclassified_bytes, uint64_t* n_unclassified);
int mic_split_device(mic_engine* e, const uint8_t* d_text, size_t nb, const uint32_t* d_rec_start, size_t n_reads, const uint32_t* d_results,
                     const uint32_t* d_norm, const mic_abund_filter* filter, int which, uint8_t* d_out, uint64_t totals[4], void* stream);
int mic_split_host(const uint8_t* text, size_t nb, const uint64_t* rec_start, size_t n_reads, const uint32_t* results, const uint32_t* norm,
                   int k, uint32_t n_targets, const mic_abund_filter* filter, int which, uint8_t* out, uint64_t totals[4]);

/* ---- hit maps: per read, the runs of k-mer assignments along it, made on the device (csrc/mic_hitmap.h: the rule, shared by host and device) ----
 * Every other output is an aggregate; a hit map says WHERE along a read the hits fall.  Read r is its packed parts as the packer wrote
 * them; part p has nk = plen - k + 1 k-mer positions, position i the 1-based label the table gives its k-mer (0: in no target, above
 * num_targets, or not this engine's to answer).  A run is a maximal stretch of equal labels inside one part.
 *   words    u32: per part, in order, one word (label << 16) | len per run (1 <= len <= 65535); between two consecutive parts one
 *            separator word 0; a read without parts has none.  A sub-part cut of a run longer than MIC_MAX_PART shows as a separator
 *            and a label run across it as two runs: the packed form cannot tell a cut from an 'N'.
 *   offsets  u32[n_reads + 1]: exclusive prefix sums of the words per read
 *   text     one line per read in input order, "<name>,<map>\n": <name> as the result CSV prints it (cut at a separator, at most 39
 *            bytes), <map> the tokens joined by single spaces - a run "<target name>:<len>" ("0:<len>" for label 0), a separator "|".
 *            exe/cuCLARK --hit-maps puts MIC_HITMAP_HEADER in front.
 * Per read the sum of len over the words with a label equals result word 0, per target the count of the sparse row, over all words
 * the sum of nk over the parts.  The map is never truncated: the kernel runs twice (count, exclusive sum, fill), a read whose result
 * row has sum 0 is not probed (its map is 0:nk per part).
 * mic_hitmap_device      the kernels alone on caller-owned device memory: packed reads as for mic_query_device, d_results the reads'
 *                        result rows, d_offsets (n_reads + 1 u32), d_words (cap_words u32).  With d_words NULL or cap_words below the
 *                        total only d_offsets and *n_words are filled (d_words is left untouched): size, then call again
 *                        (mic_ingest_fetch_packed's convention).  Synchronous on `stream` (NULL = the engine's stream).
 *                        MIC_E_UNSUPPORTED on a sharded or parted table, or when the maps need more than 2^32 - 1 words.
 * mic_hitmap_start / _stop  engine state, next to mic_split_start: from then on every mic_ingest_classify batch of this engine that
 *                        returns MIC_INGEST_OK gets its map and its text behind the query, on the slot's stream, with and without
 *                        MIC_INGEST_NO_CSV, for plain, resident and paired texts (mates are parts of the merged read).  The slot's
 *                        buffers (counts, offsets, scan storage, words, text and its pinned twin) are allocated by mic_ingest_alloc
 *                        when the maps are started by then, else with the slot's first such batch; the word and the text buffer grow
 *                        when a batch needs more and never shrink (first sizes: max_bytes / 64 words, max_bytes / 4 bytes of text).  Not started: nothing is allocated, nothing is launched.  While
 *                        started, mic_ingest_classify_group with more than one engine returns MIC_E_UNSUPPORTED; so does
 *                        mic_hitmap_start on a sharded or parted table.
 * mic_ingest_hitmap_text the text of the slot's last batch (no header line): a pointer into a pinned buffer of the slot, valid until
 *                        the slot's next call.  MIC_E_STATE when the last batch left none (handed back, or not started).
 * mic_batch_hitmap       the maps of a batch of the batch API (after mic_batch_wait; its packed reads and results are still on the
 *                        device) into host arrays: offsets (off_cap >= the batch's reads + 1, else not written), words with the
 *                        two-call sizing of mic_hitmap_device.  Synchronous.
 * mic_hitmap_runs_host   the rule's run-length encoding on the CPU (no device needed): labels per k-mer position, part after part
 *                        (label 0 or above n_targets: no target), part_nk[p] positions in part p (0: the part is skipped); returns the
 *                        number of words (written when they fit cap; words may be NULL to ask) or MIC_E_INVALID (a part of more than
 *                        65 535 positions, a null argument).
 * mic_hitmap_format      the text (no header line) of n_reads reads: read_names (the names as the indexers cut them, mic_index_reads'
 *                        [name_s, name_e); printed like mic_csv_line prints them: a name of 40 bytes or more as its first 39),
 *                        offsets, words, target names.  Returns the length (written with a terminator when it fits cap; buf may be
 *                        NULL to ask) or MIC_E_INVALID (a null name, descending offsets).  A label above n_targets prints as the
 *                        CSV's NA; the kernels never write one. */
#define MIC_HITMAP_HEADER "Object_ID,Hit_map\n"
int mic_hitmap_device(mic_engine* e, const uint32_t* d_reads_pointer, const uint16_t* d_containers, size_t n_reads, const uint32_t* d_results,
                      uint32_t* d_offsets, uint32_t* d_words, size_t cap_words, uint64_t* n_words, void* stream);
int mic_hitmap_start(mic_engine* e);
int mic_hitmap_stop(mic_engine* e);
int mic_ingest_hitmap_text(mic_engine* e, size_t slot, const uint8_t** text, uint64_t* bytes);
int mic_batch_hitmap(mic_engine* e, size_t batch, uint32_t* offsets, size_t off_cap, uint32_t* words, size_t cap_words, uint64_t* n_words);
long mic_hitmap_runs_host(const uint32_t* labels, const uint32_t* part_nk, size_t n_parts, uint32_t n_targets, uint32_t* words, size_t cap);
long mic_hitmap_format(const char* const* read_names, size_t n_reads, const uint32_t* offsets, const uint32_t* words,
                       const char* const* target_names, uint32_t n_targets, char* buf, size_t cap);

/* ---- Kraken's per-read file, made on the device (csrc/mic_kraken.h: the rule, shared by host and device) ----
 * One line per read in input order, no header line: "<C|U>\t<name>\t<taxid>\t<length>\t<map>\n".  C iff the read is classified under
 * the filter (the predicate of mic_split_start), <name> as the hit-map text prints it, <taxid> the name of target idxBest - 1 on a C
 * line (the target's label, not an LCA) and 0 on a U line, <length> the CSV's Length column (one number, merged pairs: minus one),
 * <map> the hit-map words as "<target>:<len>" tokens joined by single blanks, every separator word "|:|", an empty map "0:0".
 * mic_kraken_start / _stop   puts the engine's hit-map product (mic_hitmap_start) into this format: the same two probe passes and the
 *                        same slot buffers, another pair of text kernels.  A run has one text or the other: started while hit maps
 *                        are started (or mic_hitmap_start while this is) returns MIC_E_STATE.  Refused like hit maps
 *                        (MIC_E_UNSUPPORTED): a sharded or parted table, a group of more than one engine.  MIC_E_INVALID for a
 *                        filter mic_abundance_start would refuse.  A stop call of the format that is not on does nothing.
 * mic_ingest_kraken_text the text of the slot's last batch, as mic_ingest_hitmap_text gives the hit-map text.  MIC_E_STATE while the
 *                        hit-map format is on and when the last batch left none (handed back, or not started);
 *                        mic_ingest_hitmap_text returns MIC_E_STATE while this format is on.
 * mic_kraken_format      the text of n_reads reads on the host (no device needed): names as for mic_hitmap_format, result rows, norm
 *                        (the Length column per read; NULL: 0), the maps of mic_batch_hitmap / mic_hitmap_device.  Returns the
 *                        length (written with a terminator when it fits cap; buf may be NULL to ask) or MIC_E_INVALID (a null
 *                        argument, descending offsets, a filter that is not valid). */
int mic_kraken_start(mic_engine* e, const mic_abund_filter* filter);
int mic_kraken_stop(mic_engine* e);
int mic_ingest_kraken_text(mic_engine* e, size_t slot, const uint8_t** text, uint64_t* bytes);
long mic_kraken_format(const char* const* read_names, size_t n_reads, const uint32_t* results, const uint32_t* norm, int k, uint32_t n_targets,
                       const mic_abund_filter* filter, const uint32_t* offsets, const uint32_t* words, const char* const* target_names,
                       char* buf, size_t cap);

/* "%g" of (double)num / den for 0 < num <= den, by the integer-only formatter the device CSV kernel uses
 * (csrc/mic_fmt.h); writes at most 14 characters and a terminator, returns the length. */
int mic_format_ratio_g(uint32_t num, uint32_t den, char* out16);

/* ---- host-side pieces of the path (pure CPU, no device needed) -------------------------------- */
/* Key width rule, main.cc:274-316. */
int mic_key_bytes_rule(uint64_t htsize, int k);
/* Read indexer, CuCLARK_hh.hh:1339-1534 (one batch): fills caller arrays of capacity cap; returns the
 * number of reads (may exceed cap: call again with a larger cap), or MIC_E_INVALID if the first byte
 * is neither '>' nor '@'. */
long mic_index_reads(const uint8_t* map, size_t nb, size_t cap, uint64_t* name_s, uint64_t* name_e, uint64_t* seq_s,
                     uint64_t* seq_e, uint64_t* length);
/* Same result, indexed by n_threads OpenMP threads over byte ranges of the file (record boundaries inside a range are
 * found like the reference finds its batch starts, CuCLARK_hh.hh:1409-1471). */
long mic_index_reads_parallel(const uint8_t* map, size_t nb, int n_threads, size_t cap, uint64_t* name_s, uint64_t* name_e,
                              uint64_t* seq_s, uint64_t* seq_e, uint64_t* length);
/* Position of the first record ('>' at a line start; '@' line followed by a letters-only line and a '+' line) at or
 * after byte `from`, or nb: lets callers cut a large input into segments of whole records. */
size_t mic_find_record_start(const uint8_t* map, size_t nb, size_t from);
/* The same inside a window win[0, nb) of an input of known format (fasta != 0: FASTA, else FASTQ), from >= 1: position
 * of the first record start at or after `from`, or nb when the window holds none that can be verified. */
size_t mic_find_record_start_in(const uint8_t* win, size_t nb, int fasta, size_t from);
/* Upper bound of containers mic_pack_reads can emit for these reads. */
size_t mic_pack_bound(const uint64_t* seq_s, const uint64_t* seq_e, size_t n_reads, int k);
/* Read packer, CuCLARK_hh.hh:1616-1716.  Returns containers written or (size_t)-1 if cap is too small. */
size_t mic_pack_reads(const uint8_t* map, const uint64_t* seq_s, const uint64_t* seq_e, const uint64_t* length,
                      size_t n_reads, int k, uint32_t* reads_pointer, uint16_t* containers, size_t cap);
/* CSV, CuCLARK_hh.hh:1951-2139.  Return bytes written or -1 if cap is too small. */
int mic_csv_header(char* buf, size_t cap, int extended, const char* const* target_names, uint32_t n_targets);
int mic_csv_line(char* buf, size_t cap, const uint8_t* name, size_t name_len, uint64_t length, int paired, int k,
                 const uint32_t* result /*MIC_RESULT_WORDS*/, const char* const* target_names, uint32_t n_targets,
                 int extended, const uint32_t* row /*sparse row or NULL*/, const uint32_t* dense /*or NULL*/);

/* ---- database construction on the GPU ------------------------------------------------------
 * Builds <out_prefix>.sz/.ky/.lb from target FASTA/FASTQ files exactly as the reference's first run does
 * (makeSpecificTargetSets + RemoveCommon + Write, CuCLARK_hh.hh:691-1329, HashTableStorage_hh.hh:241-292,483-523,
 * hashTable_hh.hh:590-663): a canonical k-mer is stored iff all its occurrences belong to one label and its
 * occurrence count (saturating at 254) exceeds min_count.  target_labels[i] = label index of target_files[i]
 * (first-appearance order of the labels in the targets file).  key_bytes 0 => rule of main.cc:274-316.
 * light_gap 0 => every k-mer (cuCLARK); g > 0 => the light database of cuCLARK-l (CuCLARK_hh.hh:694-895): each maximal
 * ACGT run is cut into consecutive non-overlapping blocks of k nucleotides, numbered through the whole file, and
 * block i is used iff i % g == 0.
 * parts 0 => as many passes over disjoint bucket ranges as the free HBM requires.  Synchronous. */
int mic_db_build(const char* const* target_files, const uint16_t* target_labels, size_t n_files, int k, uint64_t htsize,
                 int key_bytes, uint32_t min_count, uint32_t light_gap, const char* out_prefix, int device, int threads,
                 uint32_t parts, uint64_t* n_kmers_out);
const char* mic_db_build_error(void);

/* ---- synthetic workload generation in HBM (bench.py / tests) ------------------- */
typedef struct mic_synth_spec {
  uint64_t seed;
  uint64_t htsize;        /* buckets                                                        */
  uint64_t genome_nt;     /* total nucleotides of the procedural genomes (~ elements)       */
  uint32_t n_targets;     /* labels; genome g (of equal length) carries label g % n_targets */
  uint32_t n_genomes;
  int32_t k;
  int32_t key_bytes;      /* 4 or 8                                                         */
  uint32_t keep_ppm;      /* 0: every k-mer of the genomes is in the database.  Otherwise a FRAGMENTED database, as the removal
                             of k-mers common to several targets leaves one (HashTableStorage_hh.hh:241-292): the k-mer start
                             positions of a genome fall into segments of geometric length (mean run_len), and a segment's k-mers
                             are kept with probability keep_ppm / 1e6                                                         */
  uint32_t run_len;       /* mean segment length in k-mer positions (0: 8)                                                    */
  uint32_t repeat_ppm;    /* 0: uniformly random genomes.  Otherwise this fraction (x 1e-6) of every genome is TANDEM REPEATS: tracts of
                             256 .. 1279 nucleotides, units of 4 .. 50; units of up to 6 nucleotides come from a pool shared by all
                             genomes (microsatellites).  The database holds what the reference's builder would keep of them: nothing that
                             lies wholly inside a shared unit's tract (common to many targets), a private unit's k-mers once          */
  uint32_t mosaic_ppm;    /* this fraction (x 1e-6) of the 2048-nucleotide segments of every genome carries MOSAIC labels: the label of
                             a k-mer there changes every 1, 2, 4 or 8 positions (close relatives after the removal of shared k-mers):
                             reads from there hit many targets with small equal counts - ties, rows of more than 15 / 64 targets       */
} mic_synth_spec;
/* Builds the on-disk-format arrays of a synthetic database in device memory the caller owns:
 *   d_sizes u8[htsize], d_keys key_bytes*[capacity], d_labels u16[capacity]; *n_elems out. */
int mic_synth_db_device(const mic_synth_spec* spec, uint8_t* d_sizes, void* d_keys, uint16_t* d_labels,
                        uint64_t capacity, uint64_t* n_elems, void* stream);
/* Builds n_reads packed reads of read_len nt in device memory (reads_pointer u32[n_reads+1],
 * containers u16[n_reads*mic_synth_read_pitch(read_len,k)]): a fraction `random_frac` are uniform random, the
 * rest are sampled from the genomes (either strand) with per-base substitution rate `sub_rate` and
 * N rate `n_rate`.  d_truth (optional, u32[n_reads*2]) receives {label+1 or 0, expected hits lower bound}. */
uint32_t mic_synth_read_pitch(uint32_t read_len, int k); /* containers reserved per read by the generator */
int mic_synth_reads_device(const mic_synth_spec* spec, uint64_t read_seed, size_t n_reads, uint32_t read_len,
                           double random_frac, double sub_rate, double n_rate, uint32_t* d_reads_pointer,
                           uint16_t* d_containers, size_t containers_cap, uint32_t* d_truth, void* stream);
/* paired != 0: every object is read 1 + 'N' + read 2 of a pair (the merged form of file.cc:205-268), 2 * read_len + 1
 * characters, containers at mic_synth_read_pitch(2 * read_len + 1, k). */
int mic_synth_reads_device2(const mic_synth_spec* spec, uint64_t read_seed, size_t n_reads, uint32_t read_len, int paired,
                            double random_frac, double sub_rate, double n_rate, uint32_t* d_reads_pointer,
                            uint16_t* d_containers, size_t containers_cap, uint32_t* d_truth, void* stream);
/* The same reads as text, one fixed-size record per read: FASTQ "@r<9 digits>\n" SEQ "\n+\n" QUAL "\n"
 * (mic_synth_text_record_bytes = 2 L + 16) or FASTA ">r<9 digits>\n" SEQ "\n" (L + 13), an N wherever the packed form ends a
 * part.  mate < 0: exactly the reads of mic_synth_reads_device (same seeds); mate 0 / 1: the two reads of a pair drawn
 * from both ends of a stretch of 2 L nucleotides (read 1 and the reverse strand's read 2), same genome, same label. */
size_t mic_synth_text_record_bytes(uint32_t read_len, int fasta);
int mic_synth_reads_text_device(const mic_synth_spec* spec, uint64_t read_seed, size_t n_reads, uint32_t read_len,
                                double random_frac, double sub_rate, double n_rate, int fasta, int mate, uint8_t* d_text,
                                size_t text_cap, void* stream);

#ifdef __cplusplus
}
#endif
#endif
