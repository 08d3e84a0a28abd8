/*
 * kvsketch.h -- C ABI of libkvsketch_hip.so, the MI355X (gfx950) sketch engine behind
 * kevlar's novel-k-mer path (count -> novel -> filter -> partition).
 *
 * The reference has no C ABI on this path: its boundary is the Python object API of khmer
 * (SURVEY.md section 8(b)).  Every entry point below names the khmer / kevlar call it
 * replaces (paths are relative to the reference tree).  Plain pointers and sizes only; no
 * torch types.  All tables live in HBM; "host" pointers are ordinary malloc'ed memory,
 * "device" pointers are HBM addresses (e.g. a torch tensor's data_ptr()).
 *
 * Conventions
 *   - every function returns KV_OK (0) or a negative KV_ERR_* code; kv_last_error() gives
 *     the message for the calling thread.
 *   - handles are owned by the caller and released with the matching *_destroy.
 *   - buffers passed in are borrowed for the duration of the call.
 *   - all work is enqueued on one HIP stream (kv_set_stream; default: the null stream) and
 *     functions that return host data synchronise that stream before returning.
 *   - calls on one sketch from several host threads are serialised by the library
 *     (kevlar/count.py:41-76 starts `numthreads` threads on one sketch + one parser).
 */
#ifndef KVSKETCH_H
#define KVSKETCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KV_OK 0
#define KV_ERR_ARG (-1)      /* bad argument (maps to ValueError)                       */
#define KV_ERR_IO (-2)       /* file cannot be opened / truncated / wrong signature      */
#define KV_ERR_TYPE (-3)     /* sketch file type does not match the requested kind        */
#define KV_ERR_HIP (-4)      /* HIP runtime failure (no device, OOM, launch failure)     */
#define KV_ERR_NOTIMPL (-5)  /* e.g. reverse_hash on a *table sketch                      */
#define KV_ERR_CAPACITY (-6) /* caller-provided buffer too small                          */

/* sketch kinds = khmer classes used at kevlar/sketch.py:14-27,99-119 */
#define KV_COUNTTABLE 0
#define KV_SMALLCOUNTTABLE 1
#define KV_NODETABLE 2
#define KV_COUNTGRAPH 3
#define KV_SMALLCOUNTGRAPH 4
#define KV_NODEGRAPH 5

#define KV_MAX_TABLES 16
#define KV_MAX_K 255       /* murmur-hashed (*table) kinds; 2-bit (*graph) kinds need k<=32 */
#define KV_MAX_SAMPLES 16  /* cases + controls in one novel scan                          */

typedef struct kv_sketch kv_sketch; /* Count-Min / Bloom tables resident in HBM            */
typedef struct kv_reads kv_reads;   /* a batch of reads, 2-bit packed, resident in HBM     */
typedef struct kv_hits kv_hits;     /* sparse result of a novel scan                       */

typedef struct kv_sketch_info {
    int32_t kind, ksize, ntables, reserved;
    uint64_t sizes[KV_MAX_TABLES]; /* khmer .hashsizes()                                   */
    uint64_t n_occupied;           /* khmer .n_occupied(): non-zero bins of table 0        */
    uint64_t n_unique;             /* khmer .n_unique_kmers() (see kv_consume)             */
    uint64_t bytes_device;         /* HBM held by the tables                               */
} kv_sketch_info;

/* ---- library / device ---------------------------------------------------------------- */
const char *kv_last_error(void);
/* Table buffers of destroyed sketches are kept for the next sketch of the same size (KV_TABLE_CACHE_GB, default 32); the library gives
 * them back by itself when one of its own allocations fails.  A host program about to allocate a large buffer of its own (torch,
 * another library) calls this first.                                                                                                */
int kv_table_cache_trim(void);
/* The library's per-stream working buffers only grow (the super-k-mer buckets of the last batch, the pair sink of an exchange owner, the
 * staging of the partitioned add): after one very large batch -- a bucket owner of a 900 M-read sample holds ~200 GB of them -- a
 * long-lived process gives them back with this call.  No other kv_* call may be running; whatever a later call kept in them (the
 * buckets a scan would reuse, an owner's combined buckets) is forgotten and rebuilt.  Also trims the table cache and the first-toucher
 * arrays of kv_unique_new.                                                                                                           */
int kv_scratch_trim(void);
const char *kv_version(void);
/* The environment variables the library looks at are one table (kevlar_amd/csrc/kv_knobs.h, kv_host.hip): SETTINGS a user may set
 * (cache sizes, host threads, progress on stderr) and TUNING switches that pin a path or shrink a geometry for tests and A/B runs --
 * same results on every path; honoured only while KV_TUNING=1 is set.  kv_knobs_describe: whole_table = 0 writes what is set right now as
 * "NAME=value ..." ("ignored:NAME=value" for a knob that is set but not honoured), 1 the table as "name<TAB>class<TAB>what it does"
 * lines.  kv_knob_get: 1 and the value if `name` is set and honoured, 0 if not, KV_ERR_ARG for a name outside the table (the Python
 * wrapper reads its own switches through this, so there is one registry).                                                           */
int kv_knobs_describe(int whole_table, char *out, uint64_t cap);
int kv_knob_get(const char *name, char *value_out, uint64_t cap);
int kv_device_count(int *n);
int kv_set_device(int device);       /* one process per GPU: call once with LOCAL_RANK; every host thread that enters the library
                                      * afterwards is switched to that GPU (HIP's current device is per thread and starts at 0)  */
/* what kv_set_device said (-1: never called), what the library last switched the CALLING thread to, what hipGetDevice says now */
int kv_thread_device_get(int *configured, int *this_thread, int *hip_current);
int kv_set_stream(void *hip_stream); /* hipStream_t for the CALLING host thread; NULL = null stream */
int kv_synchronize(void);
/* streams for host threads that count different samples at the same time (kevlar/novel.py:64-72
 * counts its samples one after the other; their kernels are independent)                     */
int kv_stream_create(void **out);
int kv_stream_destroy(void *hip_stream);

/* live per-kernel timing with HIP events on the library's stream (bench.py roofline leg).
 * kv_prof_get: accumulated milliseconds and launch count for a kernel name.             */
int kv_prof_enable(int on);
int kv_prof_reset(void);
int kv_prof_get(const char *kernel, double *ms, uint64_t *launches);
int kv_prof_names(char *buf, size_t cap); /* comma separated list of kernel names seen     */
/* kv_skm_last_instances: no reference call site; for tests.  The template instances of the super-k-mer kernels (DESIGN.md
 * section 4.1: cut, split, count, scans, route and their loose-list companions) that the last call into that front end launched on
 * the calling thread's stream, in launch order, comma separated and without blanks ("k_skm_emit_lane<1,8>,k_skm_split_sorted<3>,
 * ...": a comma between angle brackets belongs to a name).  kv_prof_get says that a family ran, this says which instance a host
 * planner chose.  Empty when that call launched none; KV_ERR_CAPACITY when the list and its terminating zero do not fit the
 * `cap` bytes of `out`.                                                                                                       */
int kv_skm_last_instances(char *out, uint64_t cap);
/* kv_bin_last_instances, kv_bin_last_plan: no reference call site; for tests.  The same report for the partitioned count (DESIGN.md
 * section 2: k_bin_hash_2bit / k_bin_hash_direct / k_bin_list, k_bin_split, k_bin_apply, k_bin_spill): the instances the last
 * partitioned count launched on the calling thread's stream -- whether it was fed by reads, by a hash list or by the super-k-mer
 * count -- in launch order, same form and same KV_ERR_CAPACITY as kv_skm_last_instances; and the numbers of that count's plan,
 * out[0..12] = T (tables), maxsl (most slices of 2^16 bins of any table), cmax (the bucket budget), F (slices per coarse bucket),
 * C (coarse buckets in use), ringB (stage B's ring entries), threadsA (stage A's workgroup size), nwgA, nwgB (writers per coarse
 * bucket / per slice), cap1, cap2 (items per private segment), weighted (0 | 1), fast4 (0 | 1).  n < 13: KV_ERR_CAPACITY.  All
 * zero when the stream's last plan failed or none was made.  The rules behind the numbers are bin_shape and bin_sizes of
 * kevlar_amd/csrc/kv_bin_plan.h, which compiles without HIP (tests/test_bin_plan.py).                                         */
int kv_bin_last_instances(char *out, uint64_t cap);
int kv_bin_last_plan(uint64_t *out, uint64_t n);

/* ---- host-side helpers (no table access) --------------------------------------------- */
/* khmer table sizing: the n largest primes below `target`, odd numbers downwards
 * (kevlar/count.py:29-35 -> khmer Counttable(k, tablesize, n)).                           */
int kv_primes_below(double target, int n, uint64_t *out, int *found);
/* khmer .hash(kmer) (kevlar/novel.py:145, kevlar/tests/test_novel.py:68-77)               */
int kv_hash_kmer(int kind, const char *kmer, int k, uint64_t *out);
/* khmer .reverse_hash(h): *graph kinds only; KV_ERR_NOTIMPL for *table kinds
 * (kevlar/tests/test_sketch.py:39-69)                                                     */
int kv_reverse_hash(int kind, uint64_t h, int k, char *out /* k+1 bytes */);
/* hash-range band of consume_seqfile_banding (kevlar/count.py:62-66): lo <= h < hi        */
int kv_band_bounds(int nbands, int band, uint64_t *lo, uint64_t *hi);

/* ---- sketches ------------------------------------------------------------------------ */
/* khmer Counttable/SmallCounttable/Nodetable/...(k, tablesize, ntables) with the primes
 * already chosen (kevlar/sketch.py:99-119, kevlar/filter.py:29)                           */
int kv_sketch_create(int kind, int ksize, int ntables, const uint64_t *sizes, kv_sketch **out);
int kv_sketch_destroy(kv_sketch *s);
/* khmer Class.load(path) / .save(path): OXLI v4 files (kevlar/sketch.py:14-27,77-92,
 * kevlar/count.py:95, kevlar/novel.py:92)                                                 */
int kv_sketch_load(const char *path, int kind, kv_sketch **out);
int kv_sketch_save(kv_sketch *s, const char *path);
/* .ksize() .n_tables() .hashsizes() .n_occupied() .n_unique_kmers()
 * (kevlar/sketch.py:62-74, kevlar/count.py:82-84)                                         */
int kv_sketch_info_get(kv_sketch *s, kv_sketch_info *out);
/* raw storage of one table, as laid out on disk (bytes / packed nibbles / packed bits)    */
int kv_sketch_table_read(kv_sketch *s, int table, uint8_t *host_out, uint64_t nbytes);
int kv_sketch_table_write(kv_sketch *s, int table, const uint8_t *host_in, uint64_t nbytes);
int kv_sketch_table_devptr(kv_sketch *s, int table, void **devptr, uint64_t *nbytes);
/* zero every table and counter (a fresh sketch of the same geometry; asynchronous)         */
int kv_sketch_clear(kv_sketch *s);
/* on != 0: the batches counted into this sketch are a CASE sample's and each is scanned right after it is counted
 * (kevlar/novel.py:92-121 loads the case samples last, then scans them).  kv_consume then also keeps, for the batch it just
 * counted, every distinct k-mer with its hash, and a kv_novel_scan of that same batch evaluates from that list instead of
 * combining and hashing the batch's k-mers a second time.  on = 2: the process counts and scans sample after sample (a server, the
 * bench's steady state), so the list is kept from the stream's very first batch on -- a one-shot run skips it there because the
 * allocation costs more than the list saves once.  Purely a performance hint: results do not depend on it. */
int kv_sketch_scan_hint(kv_sketch *s, int on);

/* ---- reads --------------------------------------------------------------------------- */
/* khmer.ReadParser stand-in (kevlar/count.py:40): the host hands over parsed sequences
 * (ASCII, concatenated; offs has n_reads+1 entries); the library 2-bit packs them into HBM.
 * Bases outside ACGT are packed as 'A' (khmer's read cleaning) and the read is flagged so
 * that the novel scan skips it (kevlar/novel.py:136-139).                                 */
int kv_reads_create(const char *bases, const uint64_t *offs, uint64_t n_reads, kv_reads **out);
/* Same, for reads that are already 2-bit packed on the host (A=0 C=1 G=2 T=3, base j of read
 * r in word r*words_per_read + j/16 at bits 2*(j%16)), all of length read_len, ACGT only.
 * Used by synthetic-read generators that never materialise ASCII.                        */
int kv_reads_create_packed(const uint32_t *words, uint64_t n_reads, uint32_t read_len, kv_reads **out);
/* Equal-length reads of a synthetic family generated ON the device (kv_synth.hip): reads [first_read, first_read +
 * n_reads) of sample 0 = proband, 1 = mother, 2 = father over an iid-uniform genome of genome_len bases; pure
 * function of (seed, sample, read index).  No reference counterpart (kevlar's test reads came from wgsim,
 * kevlar/tests/data/microtrios/README): it stands where BASELINE.json's config 4 needs 900 M reads per sample.       */
int kv_reads_generate(uint64_t genome_len, uint64_t seed, int sample, uint64_t first_read, uint64_t n_reads,
                      uint32_t read_len, double error_rate, kv_reads **out);
/* packed words [first_word, first_word + n_words) of a batch back to the host (tests; kv_reads_create_packed's layout)   */
int kv_reads_words_read(const kv_reads *r, uint64_t first_word, uint64_t n_words, uint32_t *host_out);
int kv_reads_destroy(kv_reads *r);

/* Native FASTA/FASTQ reader (gzip transparent) = khmer.ReadParser (kevlar/count.py:40,
 * kevlar/__init__.py:125-128).  kv_fastx_next parses up to max_reads records; with upload != 0 the
 * sequences are 2-bit packed into a new kv_reads batch in HBM (NULL at end of file).  The text of the
 * batch just parsed (names = header lines after '@'/'>', sequences, qualities; blobs + n+1 offsets;
 * is_fastq[i] = record had a quality line) stays valid until the next kv_fastx_next on the handle.
 * One handle may be shared by several host threads (kevlar/count.py:41-76): kv_fastx_next is
 * serialised, but then only the returned kv_reads -- not the shared batch text -- may be used.      */
typedef struct kv_fastx kv_fastx;
int kv_fastx_open(const char *path, kv_fastx **out);
int kv_fastx_next(kv_fastx *f, uint64_t max_reads, int upload, kv_reads **reads_out, uint64_t *n_reads_out);
int kv_fastx_batch_text(kv_fastx *f, const char **names, const uint64_t **name_offs, const char **seqs,
                        const uint64_t **seq_offs, const char **quals, const uint64_t **qual_offs,
                        const uint8_t **is_fastq);
int kv_fastx_num_reads(kv_fastx *f, uint64_t *n); /* khmer parser.num_reads */
/* Packed-read cache (count and novel share one parse).  With KEVLAR_PACK_CACHE=1 in the environment a
 * complete pass over FILE leaves FILE.kvpack beside it, and kv_fastx_open(FILE) streams from it when it matches the
 * source's size and mtime: kv_fastx_next then uploads the stored packed words (no inflate, no parsing);
 * kv_fastx_batch_text still gives names and all offsets, while sequences and qualities are produced per record by
 * kv_fastx_record_text (byte for byte what the source holds).  kv_fastx_from_cache tells which mode a handle is in. */
int kv_fastx_from_cache(kv_fastx *f, int *yes);
int kv_fastx_record_text(kv_fastx *f, uint64_t i, char *seq_out, char *qual_out);
/* Device ingest: a file that holds four-line FASTQ, uncompressed or as blocked gzip (BGZF: bgzip, htslib,
 * kevlar_amd.open(..., 'w')), and is read as packed batches (upload != 0) from the first call is never parsed on the host:
 * its bytes go to HBM, one wavefront inflates one BGZF member (kv_inflate.hip), lines and records are found and the
 * sequences packed by kernels (kv_fastq.hip).  kv_fastx_on_device tells whether a handle works that way; the text of a batch then
 * stays in HBM, and kv_fastx_fetch(idx, n) brings the named records to the host, after which kv_fastx_batch_text
 * describes exactly those n records.  Anything else (plain gzip, FASTA, blank lines, KV_INGEST=host) is parsed on the
 * host as before, with identical results.                                                                        */
int kv_fastx_on_device(kv_fastx *f, int *yes);
int kv_fastx_fetch(kv_fastx *f, const uint64_t *idx, uint64_t n);
int kv_fastx_close(kv_fastx *f);
int kv_reads_count(const kv_reads *r, uint64_t *n_reads, uint64_t *n_bases);
/* number of k-mers a consume of this batch visits at size k (sum over reads of len-k+1)   */
int kv_reads_num_kmers(const kv_reads *r, int ksize, uint64_t *n_kmers);

/* ---- count: sketch.consume_seqfile[_banding][_with_mask] (kevlar/count.py:43-71) ------ */
/* nbands = 0: no banding; else 0-based `band` of `nbands` (kevlar/count.py:122).
 * mask = NULL or a sketch queried with this sketch's hash:
 *   consume_masked == 0: skip the k-mer if mask.get(h) >  threshold
 *   consume_masked != 0: skip the k-mer unless mask.get(h) >= threshold
 * n_kmers_out: k-mers added.  n_unique_kmers is accumulated with the semantics of khmer's
 * multi-threaded consume (a k-mer counts as new if any of its bins was zero when ITS
 * increment landed); kv_unique_exact() gives the single-thread file-order value.   */
int kv_consume(kv_sketch *s, const kv_reads *reads, int nbands, int band, const kv_sketch *mask,
               int threshold, int consume_masked, uint64_t *n_kmers_out);
/* n_unique_kmers exactly as a single khmer thread would have counted it over `batches`
 * consumed in this order into an initially empty sketch: `s` gives the geometry, the hash
 * and k; its tables are neither read nor written, whatever they hold (needs 4 bytes of HBM
 * scratch per bin, and every batch resident).  No caller in the product any more: `kevlar
 * count` adds up kv_unique_new, batch by batch, which gives the same figure for a sketch
 * that starts empty.  Kept as public ABI and held to the oracle by the tests.             */
int kv_unique_exact(kv_sketch *s, const kv_reads *const *batches, int n_batches, int nbands,
                    int band, const kv_sketch *mask, int threshold, int consume_masked,
                    uint64_t *n_unique_out);
/* The same figure one batch at a time: *n_new_out = the k-mers of `batch` that khmer's single thread would count as new if the batch
 * were consumed into `s` now (a bin of the k-mer is clear in the tables as they stand, and no earlier k-mer of this batch touches it
 * first).  Call it before every kv_consume of the batch with the same band / mask arguments and add the results up: the sum is the
 * "distinct k-mers stored" of kevlar/count.py:82-84 for a sample of any size, no batch kept resident.                                */
int kv_unique_new(kv_sketch *s, const kv_reads *batch, int nbands, int band, const kv_sketch *mask, int threshold,
                  int consume_masked, uint64_t *n_new_out);
/* kv_unique_new keeps its first-toucher arrays (4 bytes per bin and table, ~4.5 x the sketch, one set per stream) between the batches
 * of a sample; this gives back every set no running call holds.  The wrapper calls it when a sample is done
 * (kevlar_amd.khmer: track_exact_unique(False)); kv_scratch_trim and an out-of-memory retry inside the library do the same.          */
int kv_unique_release(void);

/* ---- point queries: .get / .add on many k-mers (kevlar/filter.py:32-34,67) ------------ */
/* hash n k-mers of length k stored back to back in `kmers` (device kernel)                */
int kv_hash_kmers(int kind, const char *kmers, int k, uint64_t n, uint64_t *hashes_out);
/* the same hashes for k-mers given by position: k-mer i is reads[ann_read[i]][ann_offset[i] : + ksize].  What
 * kevlar/filter.py:32-34,67 and kevlar/readgraph.py:60-66 obtain by slicing record.ikmerseq() and calling the
 * sketch once per k-mer; here the annotated reads stay packed in HBM and only (read, offset) pairs travel.      */
int kv_hash_positions(const kv_reads *reads, int kind, int ksize, const uint32_t *ann_read, const uint32_t *ann_offset,
                      uint64_t n, uint64_t *hashes_out);
int kv_get_hashes(kv_sketch *s, const uint64_t *hashes, uint64_t n, uint8_t *counts_out);
/* adds in array order semantics are order-free (saturating); is_new_out may be NULL       */
int kv_add_hashes(kv_sketch *s, const uint64_t *hashes, uint64_t n, uint8_t *is_new_out);

/* ---- dist: khmer's abundance_distribution(parser, tracking) (kevlar/dist.py:47-77) ----------
 * In read order, a k-mer that `tracking` has not seen is recorded there and bumps
 * hist_out[counts.get(kmer)]; hist_out has 65536 entries.  Same result as the single-thread loop. */
int kv_abundance_distribution(kv_sketch *counts, kv_sketch *tracking, const kv_reads *const *batches,
                              int n_batches, uint64_t *hist_out);

/* ---- novel: the fused scan (kevlar/novel.py:21-53,123-169) ---------------------------- */
#define KV_BAND_NONE 0
#define KV_BAND_RANGE 1     /* keep k-mers whose hash lies in the band (count-side rule)     */
#define KV_BAND_REFQUIRK 2  /* reference literal: (h & (N-1)) != band0-1 -> skip
                               (kevlar/novel.py:144-147)        */
/* Scans reads[first_read:] ; a read shorter than k or flagged non-ACGT is skipped.
 * screen_thresh <= 0 disables --abund-screen.  If d_mask != NULL (device pointer, u32
 * words, zeroed by the caller) bit (read * mask_stride + offset) is set for every
 * interesting k-mer: the per-band mask that the multi-GPU merge all-reduces.             */
int kv_novel_scan(kv_sketch *const *cases, int ncase, kv_sketch *const *ctrls, int nctrl,
                  const kv_reads *reads, uint64_t first_read, int case_min, int ctrl_max,
                  int screen_thresh, int band_mode, int nbands, int band, uint32_t *d_mask,
                  uint64_t mask_stride, kv_hits **out);
/* on != 0, for the calling host thread: a kv_novel_scan (without an abundance screen) returns as soon as its kernels are done -- the
 * sketches may be cleared and counted into again -- while the hit arrays are still being copied to the host on a stream of their own;
 * kv_hits_view / kv_hits_fetch / kv_hits_shadow / kv_hits_destroy wait for them (kv_hits_count does not need to).  A caller that scans
 * batch after batch reads the hits of one scan while the next count runs.                                                          */
int kv_hits_lazy(int on);
int kv_hits_count(const kv_hits *h, uint64_t *n_hits, uint64_t *n_discarded_reads);
/* the scan's building block on its own: d_base[i] = d_counts[0] + ... + d_counts[i - 1] for i = 0 .. n (n + 1 values, the total
 * last), both DEVICE pointers; runs on the calling thread's stream and returns when it is done                              */
int kv_excl_scan_u32(const uint32_t *d_counts, uint32_t n, uint64_t *d_base);
/* copies hits sorted by (read, offset); abund has n_hits * (ncase+nctrl) entries          */
int kv_hits_fetch(const kv_hits *h, uint32_t *read, uint32_t *offset, uint8_t *abund,
                  uint64_t cap_hits, uint32_t *discarded_reads, uint64_t cap_discarded);
/* zero-copy alternative to kv_hits_fetch: pointers into the handle's (pinned) host arrays, valid until
 * kv_hits_destroy; sizes as reported by kv_hits_count                                              */
int kv_hits_view(const kv_hits *h, const uint32_t **read, const uint32_t **offset, const uint8_t **abund,
                 const uint32_t **discarded_reads);
/* --abund-screen only: interesting k-mers of DISCARDED reads that lie in front of the k-mer that tripped the screen.
 * The reference has already added them to its tally of unique novel k-mers when it drops the read
 * (kevlar/novel.py:152-164), so the summary line needs them although the reads are not reported.             */
int kv_hits_shadow(const kv_hits *h, const uint32_t **read, const uint32_t **offset, uint64_t *n);
int kv_hits_destroy(kv_hits *h);

/* ---- read-sharded multi-GPU count / scan (kevlar's banding, docs/banding.rst,
 *      kevlar/count.py:62-66, with the hashing done once per k-mer instead of once per band) ------
 * All buffer arguments named d_* are DEVICE pointers owned by the caller (bench.py and
 * kevlar_amd/shardrun.py hand in torch tensors so RCCL can move them); only kernels touch them.    */
/* Hash every k-mer of `reads` and group the hashes by the band (= rank) that owns them: d_out receives the
 * items of destination 0, then destination 1, ... back to back (cap_items >= the k-mers of the shard), the
 * layout an all-to-all with split sizes sends as it is; an item is a u64 hash or, with_tags, the pair
 * (hash, tag) with tag = (read_index_base + read) << 16 | offset and bit 63 set for reads the novel scan skips
 * (non-ACGT).  counts_out[ndest] (host) = items per destination.  kind = KV_COUNTTABLE ... selects the hash
 * function as in kv_hash_kmers.                                                                            */
int kv_route_hashes(const kv_reads *reads, int kind, int ksize, int ndest, uint64_t read_index_base,
                    int with_tags, void *d_out, uint64_t cap_items, uint64_t *counts_out);
/* kv_route_hashes for a count only, with the shard deduplicated first: an item is the pair (hash, occurrences
 * in this shard) and there is one per distinct k-mer of a super-k-mer bucket (so at most -- and at sequencing
 * coverage far fewer than -- one per k-mer; cap_items >= the k-mers of the shard still).  Same d_out layout
 * and counts_out as kv_route_hashes with two-word items.                                                    */
int kv_route_distinct(const kv_reads *reads, int kind, int ksize, int ndest, void *d_out,
                      uint64_t cap_items, uint64_t *counts_out);
/* count n (hash, count) items resident in HBM: each adds min(count, 255) to its bins, saturating -- the tables
 * end up as if the hash had been counted `count` times.  *n_added_out = sum of the counts.                  */
int kv_consume_hashes_weighted(kv_sketch *s, const void *d_items, uint64_t n, uint64_t *n_added_out);
/* (hash, occurrences) pairs as they travel between ranks: 9 bytes instead of 16.  A block of n pairs for one destination becomes
 * 1 + n + ceil(n / 8) 64-bit words -- the block's occurrences in all (exact: the statistic `kevlar count` prints), the n hashes, the n
 * occurrence counts as bytes saturated at 255 (no counter of any sketch kind holds more: `Hashtable::add` saturates).
 * kv_pairs_pack: d_pairs holds counts[0] pairs for destination 0, then counts[1] for destination 1, ...; d_out receives the blocks back
 * to back, words_per_dest[d] words each.  kv_pairs_unpack: d_in holds nsrc received blocks of words_per_src[s] words; d_pairs receives
 * their pairs as 16-byte (hash, count <= 255) items, pairs_per_src[s] each; *occurrences = the sum of the blocks' totals.              */
int kv_pairs_pack(const void *d_pairs, const uint64_t *counts, int ndest, void *d_out, uint64_t out_cap_words, uint64_t *words_per_dest);
int kv_pairs_unpack(const void *d_in, const uint64_t *words_per_src, int nsrc, void *d_pairs, uint64_t cap_pairs, uint64_t *pairs_per_src,
                    uint64_t *occurrences);
/* count n hashes resident in HBM, element i at ((uint64_t*)d_hashes)[i * stride_words]            */
int kv_consume_hashes(kv_sketch *s, const void *d_hashes, uint64_t n, uint32_t stride_words,
                      uint64_t *n_added_out);
/* kmer_is_interesting() over n_items (hash, tag) pairs; hits leave unordered as d_hit_tags[i] and
 * d_hit_abund[i * (ncase+nctrl) ...]                                                              */
int kv_novel_scan_hashes(kv_sketch *const *cases, int ncase, kv_sketch *const *ctrls, int nctrl,
                         const void *d_items, uint64_t n_items, int case_min, int ctrl_max,
                         void *d_hit_tags, void *d_hit_abund, uint64_t hit_cap, uint64_t *n_hits);
/* kv_novel_scan_hashes over the (hash, occurrences) pairs a band owner received of the case sample
 * (kv_route_distinct): an interesting pair leaves as its hash (d_hit_hashes[i]) and abundances.    */
int kv_novel_scan_distinct(kv_sketch *const *cases, int ncase, kv_sketch *const *ctrls, int nctrl,
                           const void *d_items, uint64_t n_items, int case_min, int ctrl_max,
                           void *d_hit_hashes, void *d_hit_abund, uint64_t hit_cap, uint64_t *n_hits);
/* the scan of a read shard against a known set of interesting k-mers: d_hashes[n] (entries ~0 are
 * padding) with d_abund[n * nsamples]; every k-mer of `reads` whose hash is in the set is a hit, with
 * the set's abundances; reads with non-ACGT are skipped as in kv_novel_scan; (read, offset) order.  */
int kv_novel_scan_set(const kv_reads *reads, int kind, int ksize, int nsamples, const void *d_hashes,
                      const void *d_abund, uint64_t n, kv_hits **out);
/* sort n_total gathered (tag, abundances) hits by tag; the n_valid smallest are real (padding has
 * tag ~0) and come back as an ordinary kv_hits in (read, offset) order                            */
int kv_hits_from_tagged(const void *d_tags, const void *d_abund, uint64_t n_total, uint64_t n_valid,
                        int nsamples, kv_hits **out);
/* merge nruns runs of hits: run r is rows run_starts[r] .. run_starts[r + 1] - 1 (run_starts: HOST array of nruns + 1
 * entries, the first 0) of d_read (u32), d_offset (u32) and d_abund (nsamples bytes per row); every run sorted by
 * (read, offset), the runs pairwise disjoint in (read, offset) -- the hits of the bands of a banded scan: a k-mer
 * occurrence is judged by one band.  Returns an ordinary hits handle, its list of discarded reads empty, with all rows in (read, offset)
 * order, the pair compared as one 64-bit key: any offset, any read index.  Empty runs and nruns = 1 are legal; fewer than
 * 2^32 rows in all.  A run that is not strictly ascending, or a pair that is in two runs, is the caller's error:
 * KV_ERR_ARG, no handle.                                                                           */
int kv_hits_merge(const void *d_read, const void *d_offset, const void *d_abund, const uint64_t *run_starts, int nruns,
                  int nsamples, kv_hits **out);

/* ---- partition: read graph connected components (kevlar/readgraph.py:43-84,104-137) --- */
/* One annotation = one interesting k-mer occurrence (read index in `reads`, offset).
 * node_of_read maps a read to its graph node (reads sharing a name share a node).
 * K-mers are identified by their canonical (min of forward / reverse-complement) sequence;
 * a k-mer links all nodes containing it if minabund <= #nodes <= maxabund (0 = unbounded).
 * labels_out[node] = smallest node id of its component.  n_edges_out (optional) = number
 * of distinct node pairs sharing at least one retained k-mer (networkx number_of_edges).  */
int kv_readgraph_components(const kv_reads *reads, int ksize, const uint32_t *ann_read,
                            const uint32_t *ann_offset, uint64_t n_ann,
                            const uint32_t *node_of_read, uint32_t n_nodes, uint32_t minabund,
                            uint32_t maxabund, uint32_t *labels_out, uint64_t *n_edges_out);

/* ---- augmented FASTA/FASTQ text of a batch's annotated reads (kevlar/sequence.py print_augmented_fastx) ----
 * hits (read, offset, abund[nsamples]) sorted by (read, offset); the j-th distinct read among them is record
 * rec_index[j] of the text blobs (kv_fastx_batch_text's layout).  *text_out is released with kv_text_free.   */
int kv_format_augmented(const uint32_t *hit_read, const uint32_t *hit_off, const uint8_t *abund, uint64_t n_hits,
                        int nsamples, int ksize, const uint64_t *rec_index, const char *names,
                        const uint64_t *name_offs, const char *seqs, const uint64_t *seq_offs, const char *quals,
                        const uint64_t *qual_offs, const uint8_t *is_fastq, char **text_out, uint64_t *bytes_out,
                        uint64_t *n_records_out);
int kv_text_free(char *text);

/* ---- augmented FASTA/FASTQ files as flat arrays (kevlar/sequence.pyx parse_augmented_fastx / print_augmented_fastx):
 * what `kevlar filter` (filter.py:15-82) and `kevlar partition` (readgraph.py:43-84) read and write.  A loaded file
 * exposes its records as kv_fastx_batch_text-style blobs plus, per annotation, offset and abundances (record i owns
 * annotations ann_first[i] .. ann_first[i + 1]); ksize = -1 if the stream mixes k.  kv_format_records writes any
 * selection of records / annotations back as text (see kv_augfastx.hip); release it with kv_text_free.            */
typedef struct kv_augfastx kv_augfastx;
int kv_augfastx_load(const char *path, kv_augfastx **out);
int kv_augfastx_info(const kv_augfastx *a, uint64_t *n_records, uint64_t *n_annotations, int *ksize, int *nsamples,
                     uint64_t *n_mates);
int kv_augfastx_view(const kv_augfastx *a, const char **names, const uint64_t **name_offs, const char **seqs,
                     const uint64_t **seq_offs, const char **quals, const uint64_t **qual_offs,
                     const uint8_t **is_fastq, const uint64_t **ann_first, const uint32_t **ann_offset,
                     const int32_t **ann_abund, const uint32_t **mate_record, const char **mates,
                     const uint64_t **mate_offs);
int kv_augfastx_free(kv_augfastx *a);
int kv_format_records(uint64_t n_out, const uint64_t *rec_index, const uint64_t *ann_lo, const uint64_t *ann_hi,
                      const uint32_t *ann_offset, const int32_t *ann_abund, const uint8_t *keep,
                      const int32_t *case_abund, int nsamples, int ksize, const char *names,
                      const uint64_t *name_offs, const char *seqs, const uint64_t *seq_offs, const char *quals,
                      const uint64_t *qual_offs, const uint8_t *is_fastq, const char *suffix,
                      const uint64_t *suffix_offs, const uint32_t *mate_record, uint64_t n_mates, const char *mates,
                      const uint64_t *mate_offs, char **text_out, uint64_t *bytes_out);
/* kv_format_records with the text written straight to file descriptor `fd` (a regular file, a pipe): rendered a stretch of records
 * at a time on `nthreads` host threads, written in order; *bytes_out = bytes written.  What `kevlar filter` / `kevlar partition` /
 * `kevlar novel` do with the text of print_augmented_fastx (kevlar/sequence.pyx:93-126) when their output is a plain file.  On an
 * error (an annotation outside its read, no memory, a failed write) a seekable `fd` is truncated back to where the call found it and
 * *bytes_out = 0; a pipe keeps the stretches already written (*bytes_out says how much).                                          */
int kv_format_records_fd(uint64_t n_out, const uint64_t *rec_index, const uint64_t *ann_lo, const uint64_t *ann_hi,
                         const uint32_t *ann_offset, const int32_t *ann_abund, const uint8_t *keep,
                         const int32_t *case_abund, int nsamples, int ksize, const char *names,
                         const uint64_t *name_offs, const char *seqs, const uint64_t *seq_offs, const char *quals,
                         const uint64_t *qual_offs, const uint8_t *is_fastq, const char *suffix,
                         const uint64_t *suffix_offs, const uint32_t *mate_record, uint64_t n_mates, const char *mates,
                         const uint64_t *mate_offs, int fd, int nthreads, uint64_t *bytes_out);
/* the dedup key of `kevlar partition` (kevlar/partition.py:37-47: kevlar.revcommin(read.sequence)) as two 64-bit hashes per read:
 * of the sequence or its reverse complement (complement[256]: the byte table of revcom), whichever sorts first.  Host only.     */
/* flags[i] = 1 if read i (seqs[seq_offs[i] .. seq_offs[i + 1])) holds a byte other than upper-case A, C, G, T: the packed form cannot
 * hold it, and the host hashes that read's k-mers from the text (the reference hashes every k-mer from its string).  Host only. */
int kv_reads_flag_other_bytes(const char *seqs, const uint64_t *seq_offs, uint64_t n, uint8_t *flags);
int kv_canonical_read_hashes(const char *seqs, const uint64_t *seq_offs, const uint64_t *reads, uint64_t n,
                             const uint8_t *complement, uint64_t *h1, uint64_t *h2);
/* same[j] = 1 if reads a[j] and b[j] have the same canonical sequence, min(sequence, reverse complement) by byte order: what
 * kevlar/partition.py:26-33 compares; partition confirms equal-hash pairs with it.  Host only.                                   */
int kv_canonical_reads_equal(const char *seqs, const uint64_t *seq_offs, const uint64_t *a, const uint64_t *b, uint64_t n,
                             const uint8_t *complement, uint8_t *same);

/* ---- blocked gzip (BGZF) on the device (kevlar_amd/csrc/kv_inflate.hip) --------------------------------
 * Replaces the gzip stream behind khmer.ReadParser (kevlar/__init__.py:125-128) for files whose members are
 * independent: one wavefront inflates one member.  kv_fastx_open picks this path by itself; the two
 * functions below take a whole file image in host memory (tests, tools).                                   */
int kv_bgzf_text_size(const void *file, uint64_t size, uint64_t *text_bytes, uint64_t *n_members);
int kv_bgzf_inflate_host(const void *file, uint64_t size, void *out, uint64_t out_cap, double *kernel_ms);

/* ---- ordinary gzip on the device (kevlar_amd/csrc/kv_gunzip.hip) ----------------------------------------
 * The same reader (khmer.ReadParser over a *.gz, kevlar/__init__.py:125-128) for a file that is ONE deflate
 * stream (gzip, pigz): block starts are searched for in parallel, every stretch between two starts is decoded
 * by one wavefront with the unknown 32 KB in front of it as markers, the markers are resolved by pointer
 * doubling.  kv_fastx_open picks this path by itself; this function takes a whole file image in host memory
 * and returns its text (tests, tools).  segment_text: bytes of text per pass over the device (0: 1 GB);
 * stats[4]: passes, stretches decoded, stretches dropped (false starts), stretches decoded again.
 * KV_ERR_TYPE: the stream needs the host's zlib (kv_fastx_next falls back by itself).                      */
int kv_gunzip_host(const void *file, uint64_t size, void *out, uint64_t out_cap, uint64_t segment_text,
                   uint64_t *text_bytes, uint64_t *stats, double *device_ms);

/* ---- minimizer-sharded exchange (multi-GPU count; no reference counterpart beyond banding itself, docs/banding.rst) ------
 * kevlar splits a trio over workers by k-mer band, and every worker reads every read (kevlar/count.py:62-66).  On one node
 * rank r instead holds reads [r n/N, (r+1) n/N) of every sample.  kv_mex_emit cuts its shard into super-k-mer records and
 * leaves them grouped by minimizer bucket in the caller's exchange buffer (records: plan->seg_words u64 words laid out
 * [C1][nwg1][cap1][recw]; counts: plan->cnt_entries u32, [C1][nwg1]); bucket range [c_lo[d], c_lo[d+1]) is rank d's, so one
 * all-to-all with those split points delivers every occurrence of a k-mer -- whichever shard it came from -- to one rank.
 * kv_mex_route combines what n_src ranks sent (the slabs one after the other, as all_to_all_single leaves them) at the
 * sample's full coverage and writes one (hash, occurrences) pair per distinct k-mer for the hash band's owner: the output
 * of kv_route_distinct, which the band owners add with kv_consume_hashes_weighted.  Every rank derives the same plan from
 * the sample's global size.                                                                                              */
typedef struct kv_mex_plan {
    int32_t ksize, ndest;
    uint32_t C1, F2, fbits, nwg1, cap1, recw, m, read_len;
    uint64_t seg_words, cnt_entries;
    uint64_t n_kmers_global, n_reads_global;
    uint32_t c_lo[17];
    uint32_t flags;             /* bit 0: short records (kv_mex_plan_short) */
} kv_mex_plan;
int kv_mex_plan_make(int kind, int ksize, uint64_t n_reads_global, uint32_t read_len, int ndest, kv_mex_plan *plan);
/* The same exchange with 16-byte records without positions (two thirds of the bytes a rank sends) for a sample nobody asks "where" of:
 * a control.  Not for the sample kv_mex_route(keep_scan) / kv_mex_scan_set answer the scan from.  KV_ERR_NOTIMPL when the plan's shape
 * has no such records (k > 32, a window other than k = 31's, reads beyond 224 bases): keep the plan as it is. */
int kv_mex_plan_short(kv_mex_plan *plan);
int kv_mex_emit(const kv_reads *shard, const kv_mex_plan *plan, uint64_t read_base, void *d_seg, void *d_cnt);
/* kv_mex_pack: only the filled part of the segments travels -- d_out receives it, destination after destination, and
 * records_per_dest[d] says how many records rank d gets; the counts slab travels whole, so the receiver (compact != 0 in
 * kv_mex_route) knows where every segment of every source starts.                                                        */
int kv_mex_pack(const kv_mex_plan *plan, const void *d_seg, const void *d_cnt, void *d_out, uint64_t *records_per_dest);
/* keep_scan != 0 (the case sample): the combined buckets and key + hash of every distinct k-mer stay on this stream until the next
 * call that buckets anything, for kv_mex_scan_set.                                                                          */
int kv_mex_route(const kv_mex_plan *plan, int my_dest, const void *d_recv_seg, const void *d_recv_cnt, int n_src, int compact,
                 int keep_scan, void *d_out, uint64_t cap_items, uint64_t *counts_out, uint64_t *n_kmers_in);
/* kv_mex_scan_set: the scan (kevlar/novel.py:123-169) answered by the owner of the minimizer buckets.  d_hashes[n] / d_abund[n * S]:
 * every band owner's kv_novel_scan_distinct output, all-gathered (entries ~0 are padding).  Every occurrence of a member of that
 * set among this rank's buckets leaves as d_hit_tags[i] = read << 16 | offset (global read index) with its S abundances, in
 * arbitrary order: gather them and sort with kv_hits_from_tagged.  Reads the scan skips (bytes outside ACGT) are NOT left out:
 * the caller drops their hits.  KV_ERR_CAPACITY: the state kv_mex_route(keep_scan) leaves is not there (or does not suffice);
 * scan the shard against the set instead (kv_novel_scan_set).                                                                */
int kv_mex_scan_set(int kind, int ksize, int nsamples, const void *d_hashes, const void *d_abund, uint64_t n,
                    void *d_hit_tags, void *d_hit_abund, uint64_t hit_cap, uint64_t *n_hits);
/* flags[r] bit 0: read r holds a byte outside ACGT (counted with stand-in bases, skipped by the scan); host buffer of n_reads bytes */
int kv_reads_flags(const kv_reads *reads, uint8_t *flags);
/* kv_mex_emit_pack: kv_mex_emit and kv_mex_pack in one call and one stream synchronisation.  d_out holds out_cap_words u64 words;
 * *packed = 1: the filled part fitted and sits in d_out; 0: it did not (records_per_dest is right either way), nothing was
 * written to d_out and kv_mex_pack into a buffer of plan->seg_words words does it.                                          */
int kv_mex_emit_pack(const kv_reads *shard, const kv_mex_plan *plan, uint64_t read_base, void *d_seg, void *d_cnt, void *d_out,
                     uint64_t out_cap_words, uint64_t *records_per_dest, int *packed);

/* ---- argsort for the host half of partition (kevlar/readgraph.py:123-161, kevlar/partition.py:15-55: sorted(cc), sorted by
 * size; here the array form, kevlar_amd/partition.py assemble_partitions) -------------------------------------------------
 * order[i] = index of the i-th smallest key, equal keys in index order (numpy.argsort(kind='stable')); host pointers, the
 * sort runs on the device (rocPRIM radix sort of (key, index) pairs).  kv_argsort_rows orders n rows of `width` bytes like
 * byte strings (numpy 'S<width>').                                                                                       */
int kv_argsort_u64(const uint64_t *keys, uint64_t n, uint32_t *order);
int kv_argsort_rows(const void *rows, uint64_t n, uint32_t width, uint32_t *order);

/* ---- exact seed matching for `kevlar localize` (kevlar/localize.py:113-144; kv_localize.hip) -----------------------------
 * The reference asks `bwa mem -k Z -T Z -a` for the perfect full-length matches of every contig Z-mer.  Here the canonical
 * Z-mers of the contigs (Z <= 128) become a seed set on the device and the genome text is scanned against it chunk by chunk.
 * kv_localize_create: contig c = bases[offsets[c] .. offsets[c + 1]) (ASCII, the convention of kv_reads_create); window w of the
 * contigs, counted contig after contig, gets seed_of_window[w] = the index of the first window that claimed its canonical key
 * (equal keys share an id), or 0xFFFFFFFF when the window holds a byte outside ACGT (lower case counts as upper).  n_windows must
 * be the number of windows the contigs have.
 * kv_localize_scan: one chunk of genome text whose first byte sits at global_offset of the whole text.  Every window that lies
 * inside the chunk, consists of ACGT bytes only and equals a seed or its reverse complement is reported once as
 * (ids_out[i], pos_out[i]) = (seed id, global position of the window's first byte), in no particular order.  *n_found is the
 * number of matches; when it exceeds `capacity` only `capacity` of them were written and the caller repeats the same chunk with
 * larger buffers.  Chunks overlap by Z - 1 bytes (a window belongs to the one chunk that holds all of it).  Every match also
 * counts one occurrence of its seed; the repeat of a chunk that overflowed does not count again.
 * kv_localize_counts: occurrences per seed id so far (n_windows entries; non-zero only at ids that are their own seed).
 * kv_localize_stats: for measurements only (scratch/localize_scan_rate.py), nothing of `kevlar localize` calls it: stats_out[0..3] =
 * windows of valid bases scanned, windows that passed the prefilter, matches, distinct seeds.                                      */
typedef struct kv_localize kv_localize;
int kv_localize_create(const char *bases, const uint64_t *offsets, uint64_t n_contigs, int seedsize, uint32_t *seed_of_window,
                       uint64_t n_windows, uint64_t *n_distinct, kv_localize **out);
int kv_localize_scan(kv_localize *h, const char *text, uint64_t n_bytes, uint64_t global_offset, uint32_t *ids_out,
                     uint64_t *pos_out, uint64_t capacity, uint64_t *n_found);
int kv_localize_counts(kv_localize *h, uint32_t *counts_out, uint64_t n_windows);
int kv_localize_stats(kv_localize *h, uint64_t *stats_out);
int kv_localize_destroy(kv_localize *h);

/* ---- the reference genome of `kevlar localize` / `kevlar alac` parsed on the device and kept there (kevlar/seqio.py
 * parse_seq_dict, kevlar/localize.py; kv_genome.hip) ------------------------------------------------------
 * kv_genome_open reads the file image -- uncompressed, blocked gzip (BGZF) or one gzip stream, told apart by their first bytes --,
 * inflates it on the device and splits the FASTA there.  Lines end at LF and are taken without their trailing run of space, TAB, VT,
 * FF and CR; a line whose first byte is '>' is a defline, its id the bytes behind the '>' up to the first space or TAB; a record's
 * sequence is the concatenation of the stripped lines up to the next defline; text in front of the first defline is ignored.  The
 * genome text -- the sequences in file order, one '>' byte between neighbours -- stays in one device allocation.  segment_text is the
 * number of text bytes taken per pass (0: 256 MiB; at most 1 GiB; a gzip stream's passes are as long as its decoder makes them).
 * KV_ERR_TYPE declines a file the host's text layer would read differently, and the caller parses it on the host: a byte >= 0x80, a
 * byte 0x1c-0x1f, a NUL, a CR that no LF follows, more than 4096 strippable bytes on end, an id stretch of more than 4096 bytes, a
 * gzip stream the device decoder does not take.  Duplicate ids are the caller's to refuse.
 * kv_genome_info: the number of sequences, the bytes of genome text, stats[0..3] = container (0 plain, 1 BGZF, 2 gzip), passes, bytes
 * of file text, bytes allocated for the genome text; id i = ids[id_offs[i] .. id_offs[i + 1]); sequence i = text[starts[i] ..
 * starts[i] + lengths[i]).  The arrays belong to the handle and live as long as it does; any of the pointers may be NULL.
 * kv_localize_scan_genome: kv_localize_scan over the whole resident text in one call, nothing uploaded.  The text is scanned in
 * chunks that overlap by Z - 1 bytes; chunk_bytes is the most one holds (0: the whole text in one).  A chunk begins a multiple of
 * chunk_bytes - (Z - 1) behind the text's first byte, that step rounded down to a multiple of 16 where it is 16 or more.  Matches,
 * *n_found, the overflow contract (only `capacity` matches written, the caller repeats the call with larger buffers, the repeat
 * does not count again) and the per-seed counters are those of kv_localize_scan.
 * kv_genome_fetch: n slices text[global_start[i] .. global_start[i] + len[i]) in one gather launch, clipped at the text's end; slice
 * i arrives at out[out_offs[i] .. out_offs[i + 1]) (out: room for the sum of len; out_offs: n + 1 entries).                    */
typedef struct kv_genome kv_genome;
int kv_genome_open(const char *path, uint64_t segment_text, kv_genome **out);
int kv_genome_info(kv_genome *g, uint64_t *n_seqs, uint64_t *text_bytes, uint64_t *stats, const char **ids, const uint64_t **id_offs,
                   const uint64_t **starts, const uint64_t **lengths);
int kv_localize_scan_genome(kv_localize *h, kv_genome *g, uint64_t chunk_bytes, uint32_t *ids_out, uint64_t *pos_out, uint64_t capacity,
                            uint64_t *n_found);
int kv_genome_fetch(kv_genome *g, const uint64_t *global_start, const uint64_t *len, uint64_t n, char *out, uint64_t *out_offs);
int kv_genome_close(kv_genome *g);

/* ---- calls against BED regions for `kevlar varfilter` (kevlar/varfilter.py, kevlar.parse_bed; kv_varfilter.hip) ----------------
 * The reference keeps the calls in an interval tree and looks every BED line up in it.  Here the calls become an index on the
 * device -- sorted by (chromosome, start), with the running maximum of `end` per chromosome -- and the BED text is scanned against
 * it chunk by chunk.  A region (s, e) hits a call (a, b) on a chromosome of the same name, byte for byte, iff s < e, a < e and
 * b > s (intervaltree >= 3.0.2); coordinates are 0-based half-open int64.
 * kv_varfilter_create: the distinct chromosome names of the calls, name c = names[name_off[c] .. name_off[c + 1]); call i lies on
 * chromosome call_chrom[i] at [call_start[i], call_end[i]).  A repeated name or an id out of range is KV_ERR_ARG.
 * kv_varfilter_scan: one chunk of BED text (host or device memory) that begins at a line start and ends at a line end or at the
 * end of the file; text_offset is the chunk's place in the file.  Lines end at '\n'; a line whose first byte is '#' and a line
 * of separators only (0x09-0x0d, 0x1c-0x20) are skipped; otherwise the first three tokens are chromosome, start and end, a number
 * being [+-]?[0-9]+ within int64.  A line with fewer tokens or another number makes the call KV_ERR_ARG, and
 * kv_varfilter_bad_line then gives the least file offset of such a line of that call (UINT64_MAX after a good one).
 * kv_varfilter_regions: the same join for n parsed regions (host arrays); chrom_id 0xFFFFFFFF = not among the calls' names.
 * kv_varfilter_hits: flags_out[i] = 1 if call i was hit so far, in the order the calls were given.
 * kv_varfilter_stats: stats_out[0..5] = lines seen, comment and blank lines, regions parsed, regions on a known chromosome,
 * region-call overlaps found, calls flagged.
 * kv_varfilter_plan: plan_out[0..4] = the workgroup tile (bytes) a chunk of n_bytes is scanned in, the number of tiles, the two
 * tile sizes there are and the chunk size from which the larger one is taken.  Host only.
 * kv_varfilter_chunk_cut: where a buffer of text is cut so that the chunk ends at a line end: behind its last '\n', at n_bytes
 * when the file ends with the buffer, 0 when no line ends in it (read on).  Host only.                                        */
typedef struct kv_varfilter kv_varfilter;
int kv_varfilter_create(const char *names, const uint64_t *name_off, uint64_t n_chroms, const uint32_t *call_chrom,
                        const int64_t *call_start, const int64_t *call_end, uint64_t n_calls, kv_varfilter **out);
int kv_varfilter_scan(kv_varfilter *h, const char *text, uint64_t n_bytes, uint64_t text_offset);
int kv_varfilter_bad_line(kv_varfilter *h, uint64_t *offset);
int kv_varfilter_regions(kv_varfilter *h, const uint32_t *chrom_id, const int64_t *start, const int64_t *end, uint64_t n);
int kv_varfilter_hits(kv_varfilter *h, uint8_t *flags_out, uint64_t n_calls);
int kv_varfilter_stats(kv_varfilter *h, uint64_t *stats_out);
int kv_varfilter_destroy(kv_varfilter *h);
int kv_varfilter_plan(uint64_t n_bytes, uint64_t *plan_out);
int kv_varfilter_chunk_cut(const char *buf, uint64_t n_bytes, int at_eof, uint64_t *cut);

/* ---- contig-to-cutout alignment, the first half of `kevlar call` (kevlar/alignment.pyx, src/align.c; kv_align.hip) ----------
 * The reference aligns one contig against one cutout with ksw2's extension aligner, unbanded and without z-drop: a global
 * alignment, score = H(tlen - 1, qlen - 1), traceback from that corner.  Here a batch of such jobs runs on the device and
 * reproduces score and CIGAR exactly (the rule, with its tie-breaking: DESIGN.md section 10).
 * Targets and queries are two sets of ASCII sequences, each concatenated with offsets (the convention of the seed set above).
 * Job k is jobs[3k .. 3k + 2] = (target index, query index, reverse flag); with the flag set the device aligns the reverse
 * complement of the query, which the caller therefore uploads once.  A/a C/c G/g T/t are the four bases, every other byte scores 0
 * against everything.  match, gapopen and gapextend lie in 0..127, mismatch in -127..127 (either sign means the penalty).  An
 * empty sequence, an index out of range or a score out of range is KV_ERR_ARG before anything touches the device.
 * Results per job: scores[k]; the CIGAR as run_counts[k] runs at runs[run_offsets[k] ..], in forward order, a run being
 * length << 4 | op with op 0 = M, 1 = I, 2 = D.  `runs` is one pool of `capacity` runs for the whole batch and the jobs' places in
 * it are in no particular order; *n_runs is the number of runs the batch needs, and when it exceeds `capacity` the pool's content
 * is undefined and the caller repeats the call with a larger pool.  There is no fixed 4096-character CIGAR buffer as in the
 * reference: a CIGAR is as long as it is.
 * Working memory: one direction byte per cell, padded to whole strips of KV_ALIGN_STRIP query columns (the size of one job: the
 * z_bytes call).  z_budget bounds the direction bytes alive at a time: the jobs are ordered by cell count, largest first, and cut
 * into as many launches as that takes (the plan call, host code only: order[] = the jobs in that order, launch_ends[l] = one past
 * the last position of launch l; both hold n_jobs entries).  One job that alone exceeds the budget is KV_ERR_CAPACITY.
 * The stats call is for measurements only (scratch/align_rate.py): of the last batch, stats_out[0..3] = launches, 100 MHz ticks
 * all waves spent filling, ticks they spent in traceback and copy, cells.                                                      */
#define KV_ALIGN_STRIP 256
int kv_align_z_bytes(uint32_t tlen, uint32_t qlen, uint64_t *bytes);
int kv_align_plan(const uint32_t *tlens, const uint32_t *qlens, uint64_t n_jobs, uint64_t z_budget, uint32_t *order,
                  uint64_t *launch_ends, uint64_t *n_launches);
int kv_align_batch(const char *tbases, const uint64_t *toffsets, uint64_t n_targets, const char *qbases,
                   const uint64_t *qoffsets, uint64_t n_queries, const uint32_t *jobs, uint64_t n_jobs, int match, int mismatch,
                   int gapopen, int gapextend, uint64_t z_budget, int32_t *scores, uint64_t *run_offsets, uint32_t *run_counts,
                   uint32_t *runs, uint64_t capacity, uint64_t *n_runs);
int kv_align_stats(uint64_t *stats_out);

/* ---- from alignments to calls, the second half of `kevlar call` (kevlar/cigar.py:46-71, kevlar/varmap.py:49-54, 157-161,
 * 231-317; kv_call.hip) ---------------------------------------------------------------------------------------------------
 * The reference walks every aligned base of every match block for mismatches (varmap.py:245) and searches every call's window
 * for every interesting k-mer of the contig and its reverse complement (varmap.py:309-317).  Here one batch of aligned jobs is
 * scanned on the device and every job gets one fixed-size record; the host cuts alleles and windows by slicing (DESIGN.md
 * section 11).
 * Targets, queries and jobs are those of the alignment above.  With the reverse flag set the job reads the query as
 * kevlar_amd.sequence.revcom gives it (the IUPAC codes complemented, lower case to upper, every other byte itself), reversed.
 * The CIGAR of job k is run_counts[k] runs at runs[run_offsets[k] ..] as the alignment returns them (n_runs = the size of
 * `runs`); any list of M / I / D runs of at least one base that consumes exactly both sequences is taken, each run a block.
 * Query q carries the interesting k-mers ik_offsets[q] .. ik_offsets[q + 1] of `ikmers`, each an (offset, ksize) pair in the
 * coordinates of the contig as given, whatever the strand.  ksize >= 1; mindist 0 switches the trimming off.
 * records[KV_CALL_RECORD_WORDS * k ..] of job k:
 *   [0]  1 when the tokenizer's end check folded the last block into the third-last (cigar.py:46-71), else 0
 *   [1]  the class of the block list after the end check (varmap.py:49-54): KV_CALL_NONE / KV_CALL_SNV / KV_CALL_INDEL
 *   [2 .. 8], [9 .. 15]  the scanned blocks: the match block of an snv (the second stays zero), or the left and the right flank
 *        of an indel: length; mismatches trimmed as terminal (mm < mindist or length - mm < mindist); mismatches left; the
 *        first four of those in block coordinates (0xFFFFFFFF where there is none).  A block shorter than ksize is not
 *        scanned (varmap.py:243): its counts are 0.  Bytes compare as they are, case included.  A folded block is the
 *        concatenation of its two segments, and positions are taken in that.
 *   [16 .. 24]  the IKMERS number of the calls: [16] the indel's, [17 .. 20] the SNVs of the first block, [21 .. 24] of the second
 *        (only where the block has 1 to 4 mismatches left; else 0).  The window is the reference's ALTWINDOW; an interesting
 *        k-mer counts once when its bases or their reverse complement occur anywhere in it, duplicates in the list each time.
 * An interesting k-mer that reaches past its contig or has no bases, runs that do not consume exactly both sequences, a run
 * of length 0 or of another op, an empty sequence, an index out of range: KV_ERR_ARG before anything touches the device.     */
#define KV_CALL_RECORD_WORDS 32
#define KV_CALL_NONE 0
#define KV_CALL_SNV 1
#define KV_CALL_INDEL 2
int kv_call_scan(const char *tbases, const uint64_t *toffsets, uint64_t n_targets, const char *qbases, const uint64_t *qoffsets,
                 uint64_t n_queries, const uint32_t *jobs, uint64_t n_jobs, const uint64_t *run_offsets, const uint32_t *run_counts,
                 const uint32_t *runs, uint64_t n_runs, const uint64_t *ik_offsets, const uint32_t *ikmers, int ksize, int mindist,
                 uint32_t *records);

/* ---- `kevlar simlike`: the abundances, filters and likelihoods of a batch of calls (kevlar/simlike.py:22-191, 278-300;
 * kv_simlike.hip) ----------------------------------------------------------------------------------------------------------
 * The reference asks every sketch for the counts of every window, one window and one sketch at a time, and does the rest in
 * per-k-mer Python.  Here one launch scores a batch: every call gets one fixed-size record, three doubles and its lists
 * (DESIGN.md section 12).
 * samples[0] is the case, samples[1 ..] the controls: 3 to KV_MAX_SAMPLES sketches of any kind and storage; refr is the sketch of
 * the reference genome.  All of them have k = ksize; a graph (two-bit hash) kind among them needs ksize <= 32.  Call c has the
 * alternate-allele window alt[alt_offsets[c] .. alt_offsets[c + 1]) and the reference-allele window ref[ref_offsets[c] ..
 * ref_offsets[c + 1]), both of at least ksize bases.  A k-mer is hashed as kv_hash_kmers hashes it: the bytes as they are, the
 * complement of anything outside ACGT being N, so every count is what kv_hash_kmers + kv_get_hashes give for the same bytes.
 * With nk(c) = the k-mers of call c's alt window and base(c) = the sum of nk over the calls in front of it:
 *   counts[nsamples * base(c) + s * nk(c) ..]  sample s's counts of the alt window's k-mers that the genome does not hold (refr
 *        count 0), in window order; with dropoutliers, of these the ones less than 20 away from their mean (the exact integer sum
 *        over the length, in double; an empty list stays empty)
 *   refr_abunds[base(c) ..]  windows of equal length: refr's counts of the ref window's k-mers at the positions kept by the genome
 *        test (dropoutliers does not touch them); else nothing (KV_SIMLIKE_NO_REFR), the list counting as one "none" per entry
 *        of the case's final list.  A count of 0 reads as "none" as well (kevlar/simlike.py:116).
 *   Every list has room for nk(c) entries; behind its length the room is zero.
 * records[KV_SIMLIKE_RECORD_WORDS * c ..]:
 *   [0 .. KV_MAX_SAMPLES - 1]  the final length of every sample's list (0 from nsamples on)
 *   [KV_MAX_SAMPLES]      the length of the refr-abundance list
 *   [KV_MAX_SAMPLES + 1]  DROPPED: nk(c) minus the final length of the case's list
 *   [KV_MAX_SAMPLES + 2]  flags: KV_SIMLIKE_PASSENGER no case count >= casemin; KV_SIMLIKE_CASE_ABUND caseabundlow > 0 and that many
 *        case counts < casemin on end; KV_SIMLIKE_CTRL_ABUND ctrlabundhigh > 0 and a control with more than that many counts >
 *        ctrlmax; KV_SIMLIKE_MISMATCH the list of control 1 or of control 2 is not as long as the refr-abundance list (the
 *        reference's assertion, simlike.py:136-137): the likelihoods of that call are 0 and mean nothing; KV_SIMLIKE_NO_REFR
 *   [KV_MAX_SAMPLES + 3]  nk(c)
 * likelihoods[3 * c ..] = LLDN, LLFP, LLIH (simlike.py:135-191) for mean mu, standard deviation sigma and error rate epsilon;
 *   lists are paired by position up to the shorter one; the binomial coefficient of a non-integer mu * copies is that of the
 *   floors, through lgamma.
 * Null arguments, fewer than 3 or more than KV_MAX_SAMPLES samples, a sketch of another k, a graph kind with ksize > 32, a window
 * shorter than ksize, offsets that decrease, epsilon outside (0, 1), sigma <= 0, mu < 0 or any of the three not finite:
 * KV_ERR_ARG before anything touches the device, the outputs untouched.                                                       */
#define KV_SIMLIKE_RECORD_WORDS 20
#define KV_SIMLIKE_PASSENGER 1u
#define KV_SIMLIKE_CASE_ABUND 2u
#define KV_SIMLIKE_CTRL_ABUND 4u
#define KV_SIMLIKE_MISMATCH 8u
#define KV_SIMLIKE_NO_REFR 16u
int kv_simlike_score(kv_sketch *const *samples, int nsamples, kv_sketch *refr, const char *alt, const uint64_t *alt_offsets,
                     const char *ref, const uint64_t *ref_offsets, uint64_t n_calls, int ksize, double mu, double sigma, double epsilon,
                     int casemin, int ctrlmax, int caseabundlow, int ctrlabundhigh, int dropoutliers, uint32_t *records,
                     double *likelihoods, uint8_t *counts, uint8_t *refr_abunds);

/* ---- per-partition unitigs for `kevlar assemble` (kevlar/assemble.py, kevlar/assembly.pyx; kv_assemble.hip) ------------------
 * The reference hands every partition to fermi-lite.  Here a stated rule is computed for a batch of partitions in one call
 * (DESIGN.md section 13): per partition, the canonical K-mers seen at least min_count times are the nodes of a de Bruijn graph
 * and every maximal chain of simple edges is reported once, as the smaller of the chain's sequence and its reverse complement.
 * Read r = bases[read_off[r] .. read_off[r + 1]) (ASCII, either case; a window with any other byte is skipped); partition p =
 * reads part_first[p] .. part_first[p + 1), part_first[0] = 0 and part_first[n_parts] = n_reads.  K is odd, 13..63.  A key of one
 * partition says nothing about the same key of another.
 * kv_assemble_batch computes ALL unitigs (filtering by length, ordering and naming are the caller's) and keeps them in *out;
 * *n_unitigs and *n_bases size the arrays of kv_assemble_fetch: bases_out[n_bases], offsets_out[n_unitigs + 1], part_out[n_unitigs]
 * (the partition of each unitig; unitigs come partition after partition, in no particular order inside one) and
 * count_out[n_parts] (unitigs per partition).  mem_budget bounds the device memory of one launch (0: 4 GiB): the partitions are
 * taken in order and cut into as many launches as that takes (kv_assemble_plan, host code only: launch_ends[l] = one past the last
 * partition of launch l, n_parts entries at most); one partition that alone exceeds the budget is KV_ERR_CAPACITY.
 * kv_assemble_stats: stats_out[0..6] = windows of valid bases, distinct (partition, key) pairs, solid ones, heads (oriented nodes
 * that start a unitig, both strands), unitigs, solid keys on no unitig (cycles without a head), launches.
 * Null arguments, an even K or one outside 13..63, min_count 0, offsets or partition bounds that decrease or do not cover the
 * reads: KV_ERR_ARG before anything touches the device, the outputs untouched.
 * kv_assemble_clean_batch is the same call with the graph cleaned first (rules 3a to 3c), per partition, in
 * at most clean_rounds rounds, each decided on the graph the round met: a unitig of at most tip_nodes nodes that ends in nothing
 * and hangs on a node with a stronger successor is removed (a tip), and of the unitigs of at most bubble_nodes nodes that run
 * between one pair of nodes all but the one of the highest mean count (a bubble's arms); a round that removes nothing is the
 * last.  tip_nodes = bubble_nodes = 0 is kv_assemble_batch, byte for byte and launch for launch; a limit above 0 with
 * clean_rounds 0 is KV_ERR_ARG.  The stats are over the cleaned graph ([2] counts the solid keys before cleaning, [5] the live
 * keys on no unitig).  kv_assemble_clean_stats: clean_out[0..4] = unitigs removed as tips, their keys, unitigs removed as arms,
 * their keys, removing rounds (summed over launches; a launch runs as many as the partition of it that needs the most).
 * kv_assemble_clean_plan is kv_assemble_plan for such a call: a launch that cleans takes 12 bytes more per window.              */
#define KV_ASSEMBLE_NSTATS 7
#define KV_ASSEMBLE_NCLEAN 5
typedef struct kv_assembly kv_assembly;
int kv_assemble_plan(const uint64_t *read_off, uint64_t n_reads, const uint64_t *part_first, uint64_t n_parts, int ksize,
                     uint64_t mem_budget, uint64_t *launch_ends, uint64_t *n_launches);
int kv_assemble_batch(const char *bases, const uint64_t *read_off, uint64_t n_reads, const uint64_t *part_first, uint64_t n_parts,
                      int ksize, uint32_t min_count, uint64_t mem_budget, uint64_t *n_unitigs, uint64_t *n_bases, kv_assembly **out);
int kv_assemble_clean_plan(const uint64_t *read_off, uint64_t n_reads, const uint64_t *part_first, uint64_t n_parts, int ksize,
                           uint64_t mem_budget, uint32_t tip_nodes, uint32_t bubble_nodes, uint32_t clean_rounds, uint64_t *launch_ends,
                           uint64_t *n_launches);
int kv_assemble_clean_batch(const char *bases, const uint64_t *read_off, uint64_t n_reads, const uint64_t *part_first, uint64_t n_parts,
                            int ksize, uint32_t min_count, uint64_t mem_budget, uint32_t tip_nodes, uint32_t bubble_nodes,
                            uint32_t clean_rounds, uint64_t *n_unitigs, uint64_t *n_bases, kv_assembly **out);
int kv_assemble_clean_stats(kv_assembly *h, uint64_t *clean_out);
int kv_assemble_fetch(kv_assembly *h, char *bases_out, uint64_t *offsets_out, uint32_t *part_out, uint32_t *count_out);
int kv_assemble_stats(kv_assembly *h, uint64_t *stats_out);
int kv_assemble_destroy(kv_assembly *h);

#ifdef __cplusplus
}
#endif
#endif /* KVSKETCH_H */
