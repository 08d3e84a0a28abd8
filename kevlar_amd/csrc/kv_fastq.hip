// kv_fastq.hip -- FASTQ records split and 2-bit packed on the device, fed by kv_inflate.hip.
//
// The host path (kv_fastx.hip) inflates with zlib and splits lines with memchr on one core: ~2 M reads/s from a .gz
// file, ~20 M from an uncompressed one, whatever the GPU does next.  For blocked gzip (BGZF) input the text never exists
// on the host (an uncompressed FASTQ file takes the same route minus the inflate: its bytes are uploaded as they are):
//
//   file image (mmap) --H2D, compressed--> k_inflate (one wave per member) --> text in HBM
//   k_count_lines   newlines per 16-KB chunk            \
//   k_excl_scan_u32 exclusive scan of the chunk counts    > start of every line
//   k_line_starts   byte offset of each line start      /
//   k_records       four lines = one record: checks '@' / '+', start and length of the sequence line
//   k_pack_text     2-bit packs the sequence lines into the kv_reads layout (same rules as k_pack_reads)
//
// The read lengths come back to the host (the tile table is built there, as for every batch); names, sequences and
// qualities stay in HBM until the next batch and are gathered for the few records somebody asks for
// (kv_fastq_device_fetch: the reads with interesting k-mers).  A record cut by the end of a batch is carried to the
// front of the next one.  Text that is not strict four-line FASTQ (FASTA, blank lines, wrapped sequences) is
// reported as KV_ERR_TYPE and the caller reopens the file on the host path.
//
// Replaces khmer.ReadParser over a gzip stream (kevlar/count.py:40, kevlar/novel.py:123, kevlar/__init__.py:125-128).
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "kv_device.h"
#include "kv_internal.h"
#include "kv_lines_device.h"

namespace {

#define FQ_CHUNK 16384u           // bytes per line-counting workgroup
#define FQ_THREADS 256
// k_count_lines, k_line_starts and k_record_copy: kv_lines_device.h, shared with the FASTA splitter
static_assert(FQ_CHUNK == LN_CHUNK && FQ_THREADS == LN_THREADS, "the line kernels count in chunks of LN_CHUNK bytes");

// record r = lines 4r .. 4r+3: start and length of its sequence line (a trailing '\r' is not part of a line); any
// record that does not look like FASTQ raises *bad
__global__ void k_records(const uint8_t *__restrict__ text, const uint64_t *__restrict__ line_start, uint64_t n_records,
                          uint64_t *__restrict__ seq_start, uint32_t *__restrict__ seq_len, unsigned long long *bad)
{
    for (uint64_t r = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; r < n_records; r += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t l0 = line_start[4 * r], l1 = line_start[4 * r + 1], l2 = line_start[4 * r + 2], l3 = line_start[4 * r + 3];
        uint64_t len = l2 - l1 - 1;                                  // without the newline
        if (len && text[l1 + len - 1] == '\r') --len;
        const bool ok = text[l0] == '@' && l1 - l0 >= 2 && text[l2] == '+' && l3 > l2 && len <= KV_MAX_READ_LEN;
        if (!ok) atomicMin(bad, (unsigned long long)r);
        seq_start[r] = l1;
        seq_len[r] = ok ? (uint32_t)len : 0u;
    }
}

// k_pack_reads (kv_host.hip) for sequences that sit at seq_start[r] in the text instead of back to back
__global__ void k_pack_text(const uint8_t *__restrict__ text, const uint64_t *__restrict__ seq_start, const uint32_t *__restrict__ seq_len,
                            const uint64_t *__restrict__ woff, uint64_t n_reads, uint64_t n_words, uint32_t *__restrict__ words,
                            uint32_t *__restrict__ flags32)
{
    for (uint64_t w = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; w < n_words; w += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t lo = 0, hi = n_reads;            // largest r with woff[r] <= w (empty reads share their successor's offset)
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) >> 1;
            if (woff[mid] <= w) lo = mid; else hi = mid;
        }
        const uint64_t r = lo;
        const uint64_t j0 = (w - woff[r]) * 16;
        const uint64_t len = seq_len[r];
        const uint8_t *src = text + seq_start[r] + j0;
        const uint32_t n = (uint32_t)(len - j0 < 16 ? len - j0 : 16);
        uint32_t out = 0, bad = 0;
        for (uint32_t j = 0; j < n; ++j) {
            const uint8_t c = src[j];
            uint32_t code = 0;
            if (c == 'A') code = 0;
            else if (c == 'C') code = 1;
            else if (c == 'G') code = 2;
            else if (c == 'T') code = 3;
            else { bad = 1; code = (c == 'c') ? 1u : (c == 'g') ? 2u : (c == 't') ? 3u : 0u; }
            out |= code << (2 * j);
        }
        words[w] = out;
        if (bad) atomicOr(&flags32[r >> 2], 1u << ((r & 3) * 8));
    }
}

// the last line of a file may lack its newline: give it one (the buffer has room)
__global__ void k_terminate(uint8_t *text, uint64_t n, unsigned long long *n_out)
{
    if (threadIdx.x || blockIdx.x) return;
    if (n && text[n - 1] != '\n') { text[n] = '\n'; *n_out = n + 1; }
    else *n_out = n;
}

// extents [line_start[4 idx], line_start[4 idx + 4]) of the requested records
__global__ void k_record_extents(const uint64_t *__restrict__ line_start, const uint64_t *__restrict__ idx, uint64_t n, uint64_t *__restrict__ ext)
{
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        ext[2 * i] = line_start[4 * idx[i]];
        ext[2 * i + 1] = line_start[4 * idx[i] + 4];
    }
}

}  // namespace

// device buffers of one reader; they outlive it in a small pool (a sample is usually read twice -- count, then novel --
// and hipMalloc / hipFree of gigabytes cost more than parsing a few million reads)
// Upload of a stretch of a file through pinned staging buffers.  hipMemcpyAsync from the (pageable) mapping of the file copies on
// the calling thread into the runtime's own staging buffers: ~8 GB/s per thread, 25 GB/s for three samples read side by side, half of
// what the link takes.  Here KV_STAGE_THREADS threads pread() a chunk of the file into one of three pinned buffers while the previous
// chunks are on their way (an event per buffer says when it may be filled again); the DMA then runs at the link's rate.
#define KV_STAGE_SLOTS 3
#define KV_STAGE_CHUNK (16u << 20)
struct KvStager {
    void *slot[KV_STAGE_SLOTS] = {nullptr, nullptr, nullptr};
    hipEvent_t ev[KV_STAGE_SLOTS];
    bool busy[KV_STAGE_SLOTS] = {false, false, false};
    bool ready = false, broken = false;
    bool init()
    {
        if (ready || broken) return ready;
        for (int i = 0; i < KV_STAGE_SLOTS; ++i) {
            kv_thread_device();
            if (hipHostMalloc(&slot[i], KV_STAGE_CHUNK, hipHostMallocDefault) != hipSuccess || hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) != hipSuccess) {
                (void)hipGetLastError();
                broken = true;
                return false;
            }
        }
        ready = true;
        return true;
    }
    void release()
    {
        if (!ready) return;
        for (int i = 0; i < KV_STAGE_SLOTS; ++i) { (void)hipEventSynchronize(ev[i]); (void)hipEventDestroy(ev[i]); (void)hipHostFree(slot[i]); slot[i] = nullptr; busy[i] = false; }
        ready = false;
    }
    // bytes [off, off + n) of fd to d_dst on stream st; false: nothing was issued (the caller copies from its mapping instead)
    bool upload(uint8_t *d_dst, int fd, uint64_t off, uint64_t n, hipStream_t st)
    {
        if (!init()) return false;
        int nthreads = 4;
        if (const char *e = kv_knob("KV_STAGE_THREADS")) nthreads = std::max(1, std::min(16, atoi(e)));
        int s = 0;
        for (uint64_t done = 0; done < n; done += KV_STAGE_CHUNK, s = (s + 1) % KV_STAGE_SLOTS) {
            const uint64_t len = std::min<uint64_t>(KV_STAGE_CHUNK, n - done);
            if (busy[s] && hipEventSynchronize(ev[s]) != hipSuccess) return false;
            char *dst = (char *)slot[s];
            std::vector<char> fine((size_t)nthreads, 1);
            auto fill = [&](int t) {
                uint64_t lo = len * (uint64_t)t / (uint64_t)nthreads, hi = len * (uint64_t)(t + 1) / (uint64_t)nthreads;
                while (lo < hi) {
                    const ssize_t got = pread(fd, dst + lo, (size_t)(hi - lo), (off_t)(off + done + lo));
                    if (got <= 0) { fine[(size_t)t] = 0; return; }
                    lo += (uint64_t)got;
                }
            };
            std::vector<std::thread> crew;
            for (int t = 1; t < nthreads; ++t) crew.emplace_back(fill, t);
            fill(0);
            for (std::thread &th : crew) th.join();
            for (char ok : fine) if (!ok) { kv_set_error("reading the file failed while staging it for upload"); return false; }
            if (hipMemcpyAsync(d_dst + done, dst, len, hipMemcpyHostToDevice, st) != hipSuccess) return false;
            if (hipEventRecord(ev[s], st) != hipSuccess) return false;
            busy[s] = true;
        }
        return true;
    }
};

struct FastqBuffers {
    KvArena text[2];                // the batch being served / the batch before it (the carried tail moves across)
    KvArena comp, lines, recs, scratch, fetch;
    KvGunzipArenas gz;
    KvStager stage;
    void release()
    {
        for (KvArena *a : {&text[0], &text[1], &comp, &lines, &recs, &scratch, &fetch}) a->release();
        gz.release();
        stage.release();
    }
};
namespace {
std::vector<FastqBuffers *> g_fastq_pool;
std::mutex g_fastq_pool_mu;
}

struct KvFastqDevice {
    std::string path;
    int fd = -1;
    const uint8_t *image = nullptr;
    size_t image_size = 0;
    std::vector<KvBgzfMember> members;
    size_t next_member = 0;
    bool plain = false;             // uncompressed FASTQ: the file's bytes are the text, uploaded as they are
    KvGunzip *gz = nullptr;         // an ordinary gzip stream (not BGZF): inflated a segment at a time (kv_gunzip.hip)
    uint64_t next_byte = 0;
    FastqBuffers *buf = nullptr;
    KvArena *text = nullptr;        // = buf->text
    int cur = 0;
    uint64_t carry_at = 0, carry_len = 0;     // unconsumed tail of text[cur]
    uint64_t *d_line_start = nullptr;         // of the batch being served
    uint64_t n_batch = 0;
    double bytes_per_read = 0.0;
    bool done = false;
};

static bool fq_stage_on()
{
    const char *stage_env = kv_knob("KV_STAGE");
    return !(stage_env && atoi(stage_env) == 0);
}

// bytes [off, off + n) of the file to d_dst on the stream: big stretches through the pinned staging buffers (KV_STAGE=0: straight
// from the mapping, as small ones go)
static int fq_upload(KvFastqDevice *d, uint8_t *d_dst, uint64_t off, uint64_t n, hipStream_t st)
{
    const bool staged = n >= KV_STAGE_MIN_BYTES && fq_stage_on() && d->buf->stage.upload(d_dst, d->fd, off, n, st);
    if (!staged) KV_HIP(hipMemcpyAsync(d_dst, d->image + off, n, hipMemcpyHostToDevice, st));
    return KV_OK;
}

KvFastqDevice *kv_fastq_device_open(const char *path)
{
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return nullptr;
    struct stat sb;
    if (fstat(fd, &sb) != 0 || sb.st_size < 28) { close(fd); return nullptr; }
    void *map = mmap(nullptr, (size_t)sb.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
    if (map == MAP_FAILED) { close(fd); return nullptr; }
    KvFastqDevice *d = new KvFastqDevice();
    d->path = path; d->fd = fd; d->image = (const uint8_t *)map; d->image_size = (size_t)sb.st_size;
    int yes = 0;
    if (d->image[0] == '@') d->plain = true;
    else kv_bgzf_index(d->image, d->image_size, &d->members, &yes);
    if (!yes && !d->plain) {
        const char *off = kv_knob("KV_GUNZIP");
        if (off && !strcmp(off, "host")) { kv_fastq_device_close(d); return nullptr; }
    }
    {
        std::lock_guard<std::mutex> lk(g_fastq_pool_mu);
        if (!g_fastq_pool.empty()) { d->buf = g_fastq_pool.back(); g_fastq_pool.pop_back(); }
    }
    if (!d->buf) d->buf = new FastqBuffers();
    d->text = d->buf->text;
    if (!yes && !d->plain) {
        d->gz = kv_gunzip_open(d->image, d->image_size, &d->buf->gz);
        if (!d->gz) { kv_fastq_device_close(d); return nullptr; }
        if (fq_stage_on()) {
            KvStager *stage = &d->buf->stage;
            const int fd_ = d->fd;
            kv_gunzip_set_uploader(d->gz, [stage, fd_](uint8_t *dst, uint64_t off, uint64_t n, hipStream_t st) { return stage->upload(dst, fd_, off, n, st); });
        }
    }
    return d;
}

void kv_fastq_device_close(KvFastqDevice *d)
{
    if (!d) return;
    kv_gunzip_close(d->gz);
    if (d->image) munmap((void *)d->image, d->image_size);
    if (d->fd >= 0) close(d->fd);
    if (d->buf) {
        std::lock_guard<std::mutex> lk(g_fastq_pool_mu);
        if (g_fastq_pool.size() >= 3) d->buf->gz.release();            // (the gzip inflater's buffers are gigabytes: three sets are kept, a trio read side by side)
        if (g_fastq_pool.size() < 4) g_fastq_pool.push_back(d->buf);
        else { d->buf->release(); delete d->buf; }
    }
    delete d;
}

// ---- kv_fastq_device_next: select input -> text on the device -> count lines -> decide -> line starts and records -> deliver
// what the steps of a batch share
struct FqBatch {
    KvFastqDevice *d;
    hipStream_t st;
    KvLap lap;                      // wall time of the steps of a batch on stderr
    uint64_t max_reads, text_cap, want;
    double per_read;
    // this attempt's input: members [m0, m1) or bytes [b0, b0 + fresh) of the file, or a gunzip segment of `fresh` bytes of text
    size_t m0 = 0, m1 = 0;
    uint64_t b0 = 0, fresh = 0, total_in = 0;
    bool final = false;             // the file ends with it
    int nxt = 0;                    // the text buffer it is built in
    uint8_t *text = nullptr;
    uint32_t n_chunks = 0;
    uint64_t *d_base = nullptr;     // lines in front of every chunk
    unsigned long long total = 0, n_lines = 0;
    FqBatch(KvFastqDevice *d_, hipStream_t st_, uint64_t max_reads_) : d(d_), st(st_), lap("[kv_ingest] ", 22, st_), max_reads(max_reads_)
    {
        const char *cap_env = kv_knob("KV_INGEST_TEXT_MB");            // tests shrink the batches
        text_cap = (cap_env ? strtoull(cap_env, nullptr, 10) : 4096ull) << 20;
        per_read = d->bytes_per_read > 0 ? d->bytes_per_read : 280.0;
        want = std::min<uint64_t>((uint64_t)((double)max_reads * per_read * 1.02) + 65536, text_cap);
    }
};

// members (or, for an uncompressed file, bytes; or a decoded gunzip segment) of this attempt
static int fq_select(FqBatch &b)
{
    KvFastqDevice *d = b.d;
    b.m0 = b.m1 = d->next_member;
    b.fresh = 0;
    b.b0 = d->next_byte;
    bool gz_last = false;
    if (d->gz) {
        const uint64_t ask = b.want > d->carry_len + (1u << 20) ? b.want - d->carry_len : (1u << 20);
        KV_STEP(kv_gunzip_decode(d->gz, ask + ask / 20, &b.fresh, &gz_last));
    } else if (d->plain) {
        b.fresh = std::min<uint64_t>(d->image_size - b.b0, b.want > d->carry_len + 65536 ? b.want - d->carry_len : 65536);
    } else {
        while (b.m1 < d->members.size() && (b.m1 == b.m0 || d->carry_len + b.fresh + d->members[b.m1].isize <= b.want)) b.fresh += d->members[b.m1++].isize;
    }
    b.lap(d->gz ? "gunzip: decode" : "select");
    b.final = d->gz ? gz_last : d->plain ? b.b0 + b.fresh == d->image_size : b.m1 == d->members.size();
    b.total_in = d->carry_len + b.fresh;
    return KV_OK;
}

// the carried tail of the previous batch, then the fresh text behind it: uploaded, emitted by the gunzip decoder or inflated
static int fq_text(FqBatch &b)
{
    KvFastqDevice *d = b.d;
    hipStream_t st = b.st;
    b.nxt = d->cur ^ 1;
    KV_HIP(d->text[b.nxt].need(kv_round_up(b.total_in + 64, 4096)));
    uint8_t *text = b.text = (uint8_t *)d->text[b.nxt].p;
    if (d->carry_len) KV_HIP(hipMemcpyAsync(text, (const uint8_t *)d->text[d->cur].p + d->carry_at, d->carry_len, hipMemcpyDeviceToDevice, st));
    if (d->plain && b.fresh) KV_STEP(fq_upload(d, text + d->carry_len, b.b0, b.fresh, st));
    if (d->gz && b.fresh) KV_STEP(kv_gunzip_emit(d->gz, text + d->carry_len));
    if (b.m1 > b.m0) {
        const uint64_t c0 = d->members[b.m0].in_off, c1 = d->members[b.m1 - 1].in_off + d->members[b.m1 - 1].in_len;
        // (a damaged member is read at most ~600 bytes past its end before k_inflate catches it: one dynamic block
        // header, or one row of a stored block; the slack is zeroed so that what it decodes there is an error, not noise)
        KV_HIP(d->buf->comp.need(kv_round_up(c1 - c0 + KV_INFLATE_SLACK, 4096)));
        KV_STEP(fq_upload(d, (uint8_t *)d->buf->comp.p, c0, c1 - c0, st));
        KV_HIP(hipMemsetAsync((uint8_t *)d->buf->comp.p + (c1 - c0), 0, KV_INFLATE_SLACK, st));
        std::vector<uint64_t> text_off(b.m1 - b.m0);
        uint64_t at = d->carry_len;
        for (size_t i = b.m0; i < b.m1; ++i) { text_off[i - b.m0] = at; at += d->members[i].isize; }
        KV_STEP(kv_bgzf_inflate((const uint8_t *)d->buf->comp.p, c0, d->members.data() + b.m0, b.m1 - b.m0, text_off.data(), text, d->buf->scratch));
    }
    b.lap("text on the device");
    return KV_OK;
}

// newlines per chunk and in front of every chunk; the last line of a file gets its newline first
static int fq_count_lines(FqBatch &b)
{
    hipStream_t st = b.st;
    b.n_chunks = (uint32_t)((b.total_in + 1 + FQ_CHUNK - 1) / FQ_CHUNK);
    KvCarve<3> scratch({(uint64_t)b.n_chunks * 4, ((uint64_t)b.n_chunks + 1) * 8, 256});
    KV_HIP(scratch.from(b.d->buf->scratch));
    uint32_t *d_counts = scratch.at<uint32_t>(0);
    b.d_base = scratch.at<uint64_t>(1);
    unsigned long long *d_ctr = scratch.at<unsigned long long>(2);
    b.total = b.total_in;
    if (b.final) {
        hipLaunchKernelGGL(k_terminate, dim3(1), dim3(1), 0, st, b.text, b.total_in, d_ctr);
        KV_HIP(hipMemcpyAsync(&b.total, d_ctr, 8, hipMemcpyDeviceToHost, st));
        KV_HIP(hipStreamSynchronize(st));
    }
    {
        KvProfScope prof("k_count_lines");
        hipLaunchKernelGGL(k_count_lines, dim3(b.n_chunks), dim3(FQ_THREADS), 0, st, (const uint8_t *)b.text, (uint64_t)b.total, d_counts);
        kv_excl_scan_launch(d_counts, b.n_chunks, b.d_base, st);
    }
    KV_HIP(hipGetLastError());
    KV_HIP(hipMemcpyAsync(&b.n_lines, b.d_base + b.n_chunks, 8, hipMemcpyDeviceToHost, st));
    KV_HIP(hipStreamSynchronize(st));
    return KV_OK;
}

// what becomes of the text now that its lines are counted
enum FqVerdict {
    FQ_SERVE,          // its first n whole records are the batch (n = 0 with the file at its end: nothing but a blank tail)
    FQ_MORE_GUNZIP,    // fewer records than asked for: the text waits as the carry and another gunzip segment joins it
    FQ_MORE_INPUT,     // not one whole record: the members (bytes) go back and the budget doubles
    FQ_END,            // blank lines behind the last record: the file is over
    FQ_CUT_RECORD      // the file ends inside a record
};
static int fq_decide(const FqBatch &b, uint64_t n, FqVerdict *verdict)
{
    const KvFastqDevice *d = b.d;
    *verdict = FQ_SERVE;
    // the segment held fewer records than asked for (its size is a guess from the compression ratio so far) and the text budget is
    // not spent
    if (d->gz && !b.final && b.n_lines / 4 < b.max_reads && (b.total_in < b.text_cap || b.n_lines < 4)) *verdict = FQ_MORE_GUNZIP;
    else if (n == 0 && !b.final) *verdict = FQ_MORE_INPUT;      // (huge records or a tiny budget)
    else if (n == 0 && b.final && b.n_lines % 4 != 0) {
        // blank lines behind the last record (a common way for a FASTQ file to end) are not a partial record: the few
        // bytes are looked at on the host; only a genuinely cut record sends the file to the host parser
        bool blank = b.total_in <= 4096;
        if (blank) {
            unsigned char tail[4096];
            KV_HIP(hipMemcpyAsync(tail, b.text, b.total_in, hipMemcpyDeviceToHost, b.st));
            KV_HIP(hipStreamSynchronize(b.st));
            for (uint64_t i = 0; i < b.total_in && blank; ++i) blank = tail[i] == '\n' || tail[i] == '\r' || tail[i] == ' ' || tail[i] == '\t';
        }
        *verdict = blank ? FQ_END : FQ_CUT_RECORD;
    }
    return KV_OK;
}

// the start of every line of the first n records, each record checked and measured; the reader's state moves on to this batch
static int fq_records(FqBatch &b, uint64_t n, uint64_t **d_seq_start, uint32_t **d_seq_len, std::vector<uint32_t> *lens)
{
    KvFastqDevice *d = b.d;
    hipStream_t st = b.st;
    KV_HIP(d->buf->lines.need(kv_round_up((4 * n + 2) * 8, 256)));
    uint64_t *line_start = (uint64_t *)d->buf->lines.p;
    KV_HIP(hipMemsetAsync(line_start, 0, 8, st));
    KvCarve<3> recs({n * 8, n * 4, 256});
    KV_HIP(recs.from(d->buf->recs));
    *d_seq_start = recs.at<uint64_t>(0);
    *d_seq_len = recs.at<uint32_t>(1);
    unsigned long long *d_bad = recs.at<unsigned long long>(2);
    KV_HIP(hipMemsetAsync(d_bad, 0xFF, 8, st));
    {
        KvProfScope prof("k_line_starts");
        hipLaunchKernelGGL(k_line_starts, dim3(b.n_chunks), dim3(FQ_THREADS), 0, st, (const uint8_t *)b.text, (uint64_t)b.total, (const uint64_t *)b.d_base,
                           (uint64_t)(4 * n), line_start);
    }
    {
        KvProfScope prof("k_records");
        hipLaunchKernelGGL(k_records, dim3((unsigned)std::min<uint64_t>((n + 255) / 256, 8192)), dim3(256), 0, st, (const uint8_t *)b.text,
                           (const uint64_t *)line_start, n, *d_seq_start, *d_seq_len, d_bad);
    }
    KV_HIP(hipGetLastError());
    lens->resize(n);
    unsigned long long bad = 0, consumed = 0;
    KV_HIP(hipMemcpyAsync(lens->data(), *d_seq_len, n * 4, hipMemcpyDeviceToHost, st));
    KV_HIP(hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, st));
    KV_HIP(hipMemcpyAsync(&consumed, line_start + 4 * n, 8, hipMemcpyDeviceToHost, st));
    KV_HIP(hipStreamSynchronize(st));
    if (bad != ~0ull) {
        kv_set_error("%s: record %llu of the batch is not four-line FASTQ", d->path.c_str(), bad);
        return KV_ERR_TYPE;
    }
    d->carry_at = consumed;
    d->carry_len = b.total - consumed;
    if (b.final && d->carry_len == 0) d->done = true;
    d->bytes_per_read = (double)consumed / (double)n;
    d->d_line_start = line_start;
    d->n_batch = n;
    b.lap("lines and records");
    return KV_OK;
}

int kv_fastq_device_next(KvFastqDevice *d, uint64_t max_reads, kv_reads **reads_out, uint64_t *n_out)
{
    *n_out = 0;
    *reads_out = nullptr;
    if (d->done) return KV_OK;             // (the batch served last stays served: its records can still be fetched)
    FqBatch b(d, kv_stream(), max_reads);
    for (;;) {
        KV_STEP(fq_select(b));
        if (b.total_in == 0) { d->done = true; return KV_OK; }     // end of file: nothing of the previous batch has been touched
        // (the batch served last -- its text buffer, its line starts, n_batch -- stays fetchable until a NEW batch with records
        // in it has been produced: a caller that kept it asks once more only to learn that the file has ended, and a file that
        // ends in blank lines gets here with a carry of a byte or two)
        KV_STEP(fq_text(b));
        KV_STEP(fq_count_lines(b));
        const uint64_t n = std::min<uint64_t>(b.n_lines / 4, max_reads);
        FqVerdict verdict;
        KV_STEP(fq_decide(b, n, &verdict));
        switch (verdict) {
        case FQ_MORE_GUNZIP: {
            const uint64_t have = b.n_lines / 4;
            const double each = have ? (double)b.total_in / (double)have : b.per_read;
            d->n_batch = 0;               // the other text buffer -- the previous batch's -- is written next
            d->cur = b.nxt;
            d->carry_at = 0;
            d->carry_len = b.total_in;
            b.want = std::min<uint64_t>(b.total_in + (uint64_t)((double)(max_reads - have) * each * 1.05) + (1u << 20), std::max<uint64_t>(b.text_cap, b.total_in + (1u << 20)));
            continue;
        }
        case FQ_MORE_INPUT:
            d->next_member = b.m0;
            d->next_byte = b.b0;
            b.want = b.want * 2 + 65536;
            continue;
        case FQ_CUT_RECORD:
            kv_set_error("%s ends inside a FASTQ record", d->path.c_str());
            return KV_ERR_TYPE;
        case FQ_END:
            d->done = true; d->carry_len = 0;
            return KV_OK;
        case FQ_SERVE:
            break;
        }
        d->next_member = b.m1;
        d->next_byte = b.b0 + (d->plain ? b.fresh : 0);
        if (n == 0) { d->done = true; d->carry_len = 0; return KV_OK; }      // blank tail: the previous batch is still the current one
        d->cur = b.nxt;
        d->n_batch = 0;
        uint64_t *d_seq_start = nullptr;
        uint32_t *d_seq_len = nullptr;
        std::vector<uint32_t> lens;
        KV_STEP(fq_records(b, n, &d_seq_start, &d_seq_len, &lens));
        KV_STEP(kv_reads_from_device_text(b.text, d_seq_start, d_seq_len, lens.data(), n, reads_out));
        b.lap("packed batch");
        *n_out = n;
        return KV_OK;
    }
}

// launches k_pack_text for kv_reads_from_device_text (kv_host.hip owns the kv_reads layout)
void kv_fastq_pack_launch(const uint8_t *d_text, const uint64_t *d_seq_start, const uint32_t *d_seq_len, const uint64_t *d_woff, uint64_t n_reads,
                          uint64_t n_words, uint32_t *d_words, uint32_t *d_flags32, hipStream_t st)
{
    KvProfScope prof("k_pack_text");
    const unsigned grid = (unsigned)std::min<uint64_t>((n_words + 255) / 256, 65536);
    hipLaunchKernelGGL(k_pack_text, dim3(grid), dim3(256), 0, st, d_text, d_seq_start, d_seq_len, d_woff, n_reads, n_words, d_words, d_flags32);
}

int kv_fastq_device_fetch(KvFastqDevice *d, const uint64_t *idx, uint64_t n, std::string *blob, std::vector<uint64_t> *offs)
{
    blob->clear();
    offs->assign(1, 0);
    if (n == 0) return KV_OK;
    for (uint64_t i = 0; i < n; ++i)
        KV_REQUIRE(idx[i] < d->n_batch, KV_ERR_ARG, "record %llu is not in the current batch of %llu", (unsigned long long)idx[i], (unsigned long long)d->n_batch);
    hipStream_t st = kv_stream();
    KvCarve<3> fetch({n * 8, n * 16, n * 8});
    KV_HIP(fetch.from(d->buf->fetch));
    uint64_t *d_idx = fetch.at<uint64_t>(0), *d_ext = fetch.at<uint64_t>(1), *d_dst = fetch.at<uint64_t>(2);
    KV_HIP(hipMemcpyAsync(d_idx, idx, n * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_record_extents, dim3((unsigned)std::min<uint64_t>((n + 255) / 256, 4096)), dim3(256), 0, st, (const uint64_t *)d->d_line_start,
                       (const uint64_t *)d_idx, n, d_ext);
    KV_HIP(hipGetLastError());
    std::vector<uint64_t> ext(2 * n);
    KV_HIP(hipMemcpyAsync(ext.data(), d_ext, n * 16, hipMemcpyDeviceToHost, st));
    KV_HIP(hipStreamSynchronize(st));
    offs->resize(n + 1);
    for (uint64_t i = 0; i < n; ++i) (*offs)[i + 1] = (*offs)[i] + (ext[2 * i + 1] - ext[2 * i]);
    const uint64_t bytes = (*offs)[n];
    uint8_t *d_out = nullptr;
    KV_HIP(kv_hip_malloc((void **)&d_out, bytes + 16));
    hipError_t e = hipMemcpyAsync(d_dst, offs->data(), n * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_record_copy, dim3((unsigned)std::min<uint64_t>(n, 16384)), dim3(64), 0, st, (const uint8_t *)d->text[d->cur].p, (const uint64_t *)d_ext,
                           (const uint64_t *)d_dst, n, d_out);
        e = hipGetLastError();
    }
    blob->resize(bytes);
    if (e == hipSuccess) e = hipMemcpyAsync(&(*blob)[0], d_out, bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(d_out);
    if (e != hipSuccess) { kv_set_error("kv_fastq_device_fetch: %s", hipGetErrorString(e)); return KV_ERR_HIP; }
    return KV_OK;
}
