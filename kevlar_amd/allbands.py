"""`kevlar novel --num-bands N --all-bands`: every k-mer band in ONE run, the bands' hits merged on the device.

K-mer banding (docs/banding.rst) is how kevlar fits a sample whose sketches do not fit in memory: N passes with
sketches of 1/N the size, then `kevlar unband` over the N outputs.  Run the reference way that is N processes, N
augmented FASTQ files and a merge that parses the text back and folds it by read name.  Here one command counts and
scans band after band -- the bands of a rank one after the other, the ranks of a torch.distributed launch side by
side, rank r taking bands r, r + W, ... -- keeps each band's sparse hits (read, offset, abundances) per scan batch on
the host, and then walks the case reads once more: the runs of a batch go to the device (from every rank to rank 0),
kv_hits_merge ranks them into (read, offset) order, and the batch's annotated reads are written, in input order.
As a set of records the output is `kevlar unband` over the N per-band outputs of the same arguments.

Every rank reads and hashes every read (that is banding; the read-sharded exchange of kevlar_amd.shardrun is another
layout): W GPUs buy memory per GPU and bands running side by side, not ingest.

A rank whose band work fails does not leave the others waiting: it enters the next gather with a negative count
(shardrun.PeerDeclined), every rank learns it at that collective, the reasons are exchanged and all of them stop."""
import os
from types import SimpleNamespace

import numpy as np

import kevlar_amd
from kevlar_amd import _lib, khmer, novel
from kevlar_amd.sketch import KevlarUnsuitableFPRError

MAX_RANKS = 16
_REASON_BYTES = 512


class AllBandsFailed(RuntimeError):
    """a rank could not do its part of an --all-bands run; every rank raises this, naming the ranks and their reasons"""


def band_plan(numbands, world=1, rank=0):
    """the bands (0-based) rank `rank` of `world` takes, in the order it takes them"""
    return list(range(rank, numbands, world))


def _test_failure(rank, band):
    """tests: KV_ALLBANDS_TEST_FAIL='<rank>:<band>' (band 0-based) makes that rank fail before it counts that band"""
    if _lib.knob('KV_ALLBANDS_TEST_FAIL', '') == '{}:{}'.format(rank, band):
        raise _lib.KvError(_lib.KV_ERR_HIP, 'forced by KV_ALLBANDS_TEST_FAIL')


def _after_skip(batches, skipuntil):
    """(text, first read) of the batches a scan with --skip-until looks at: as novel._scan, without a word to the log"""
    for text in batches:
        start = 0
        if skipuntil:
            at = text.find_name(skipuntil)
            if at < 0:
                text.batch.close()
                continue
            skipuntil, start = None, at + 1
        yield text, start


class _Ranks(object):
    """the ranks of the run and what they say to each other; world 1 = this process alone, nothing is sent"""

    def __init__(self, group):
        self.group, self.world, self.rank, self.staged, self.failure = group, 1, 0, False, None
        if group is not None:
            import torch.distributed as dist
            import torch
            self.world, self.rank = dist.get_world_size(group), dist.get_rank(group)
            # gloo moves host tensors (ranks sharing a device); a group with both transports takes RCCL if every rank has a device
            backend = str(dist.get_backend(group))
            self.staged = backend == 'gloo' or (backend != 'nccl' and torch.cuda.device_count() < self.world)

    def fail(self, exc):
        """this rank cannot go on; alone it stops here, among others it says so inside the next gather"""
        if self.world == 1:
            raise exc
        if self.failure is None:
            self.failure = exc

    def gather(self, rows, n_valid):
        """every rank's first n_valid rows (shardrun.gather_rows); a rank that has failed brings a negative count instead, and
        every rank leaves the collective with AllBandsFailed"""
        from kevlar_amd import shardrun
        try:
            return shardrun.gather_rows(rows, -1 if self.failure is not None else n_valid, 0, self.group, self.staged)
        except shardrun.PeerDeclined:
            raise AllBandsFailed(self._reasons()) from self.failure

    def _reasons(self):
        """one more collective after a declined gather: what each failed rank has to say, known to all"""
        import torch
        import torch.distributed as dist
        said = b'' if self.failure is None else '{}: {}'.format(type(self.failure).__name__, self.failure).encode('utf-8', 'replace')
        mine = np.zeros(_REASON_BYTES, dtype=np.uint8)
        mine[:min(len(said), _REASON_BYTES)] = np.frombuffer(said[:_REASON_BYTES], dtype=np.uint8)
        device = torch.device('cpu') if self.staged else torch.device('cuda', torch.cuda.current_device())
        everyone = torch.empty(self.world * _REASON_BYTES, dtype=torch.uint8, device=device)
        dist.all_gather_into_tensor(everyone, torch.from_numpy(mine).to(device), group=self.group)
        everyone = everyone.cpu().numpy().reshape(self.world, _REASON_BYTES)
        lines = []
        for r in range(self.world):
            text = everyone[r].tobytes().rstrip(b'\0').decode('utf-8', 'replace')
            if text:
                lines.append('rank {} failed: {}'.format(r, text))
        return '--all-bands stops on every rank; ' + '; '.join(lines)


def _band_hits(casefiles, controlfiles, ksize, memory, maxfpr, numbands, band, casemin, ctrlmax, abundscreen, skipuntil, numthreads,
               batchsize):
    """Count band `band` of every sample and scan the case reads against it: (the hits of every scan batch as host copies
    (read, offset, abund), instances, unique novel k-mers).  The band's sketches are gone when this returns."""
    args = SimpleNamespace(control=controlfiles, case=casefiles, control_counts=None, case_counts=None, save_ctrl_counts=None,
                           save_case_counts=None, ksize=ksize, memory=memory, max_fpr=maxfpr, num_bands=numbands, threads=numthreads)
    kept = {} if not _lib.knob('KV_NOVEL_REREAD') else None
    controls, cases = novel._load(args, band, kept, kevlar_amd.Timer())
    case_reads = kevlar_amd.multi_file_iter_khmer([path for files in casefiles for path in files], kept=kept)
    runs, hashes, instances = [], [], 0
    for text, hits, _ in novel._scan(case_reads, cases, controls, ksize, abundscreen, casemin, ctrlmax, numbands, band, skipuntil, False,
                                     batchsize):
        reads, offsets, abunds, dropped = hits
        if len(reads):
            hashes.append(cases[0].hash_positions(text.batch, reads, offsets))
            instances += len(reads)
        if len(dropped) and len(dropped.shadow[0]):       # the k-mers of a screened read in front of the one that tripped the screen
            hashes.append(cases[0].hash_positions(text.batch, dropped.shadow[0], dropped.shadow[1]))
        text.batch.close()
        runs.append((np.array(reads, dtype=np.uint32), np.array(offsets, dtype=np.uint32), np.array(abunds, dtype=np.uint8)))
    return runs, instances, len(np.unique(np.concatenate(hashes))) if hashes else 0


def _rows(runs, S):
    """the runs of one batch as one block of rows: read and offset as four little-endian bytes each, then the S abundances"""
    n = sum(len(r[0]) for r in runs)
    rows = np.zeros((n, 8 + S), dtype=np.uint8)
    at = 0
    for reads, offsets, abunds in runs:
        m = len(reads)
        rows[at:at + m, 0:4] = reads.astype('<u4').view(np.uint8).reshape(m, 4)
        rows[at:at + m, 4:8] = offsets.astype('<u4').view(np.uint8).reshape(m, 4)
        rows[at:at + m, 8:] = abunds.reshape(m, S)
        at += m
    return rows


def _merge(d_rows, lengths, S):
    """rows on the device (torch uint8 [n, 8 + S]; runs of `lengths` rows back to back) -> hits in (read, offset) order"""
    import torch
    starts = np.concatenate(([0], np.cumsum(np.asarray(lengths, dtype=np.uint64)))).astype(np.uint64)
    d_read = d_rows[:, 0:4].contiguous()
    d_offset = d_rows[:, 4:8].contiguous()
    d_abund = d_rows[:, 8:].contiguous()
    torch.cuda.current_stream().synchronize()         # the library reads them on its own stream (shardrun: stream invariant)
    return khmer.hits_merge(d_read.data_ptr(), d_offset.data_ptr(), d_abund.data_ptr(), starts, S)


def novel_all_bands(casefiles, controlfiles, ksize, memory, maxfpr, numbands, casemin, ctrlmax, abundscreen=None, skipuntil=None,
                    numthreads=1, batchsize=novel.SCAN_BATCH_READS, group=None, tally=None):
    """Yield, batch by batch of the case reads, the augmented FASTA/FASTQ text (bytes) of the reads that hold an interesting
    k-mer in ANY of the `numbands` bands, each with all of its annotations in offset order: `kevlar unband` over the
    per-band outputs, in input order.  casefiles / controlfiles: one list of paths per sample; memory: bytes per sample
    sketch of ONE band.  group: a torch.distributed process group whose ranks share the bands (None: this process takes
    them all); every rank must iterate to the end, only rank 0 is given text.  tally (a dict) receives `instances`,
    `kmers` and `reads` of the closing log line, which rank 0 prints."""
    import torch
    clock = kevlar_amd.Timer()
    clock.start()
    ranks = _Ranks(group)
    S = len(casefiles) + len(controlfiles)
    device = torch.device('cuda', torch.cuda.current_device())
    mine = band_plan(numbands, ranks.world, ranks.rank)
    per_band, instances, kmers = [], 0, 0
    for band in mine:
        if ranks.failure is not None:
            break
        kevlar_amd.plog('[kevlar::novel] band {:d}/{:d}'.format(band + 1, numbands))
        try:
            _test_failure(ranks.rank, band)
            runs, found, unique = _band_hits(casefiles, controlfiles, ksize, memory, maxfpr, numbands, band, casemin, ctrlmax,
                                             abundscreen, skipuntil, numthreads, batchsize)
        except (Exception, KevlarUnsuitableFPRError) as exc:
            ranks.fail(exc)
            break
        if per_band and len(runs) != len(per_band[0]):
            ranks.fail(AllBandsFailed('band {} was scanned in {} batches, band {} in {}'.format(band + 1, len(runs), mine[0] + 1, len(per_band[0]))))
            break
        per_band.append(runs)
        instances += found
        kmers += unique

    # ---- merge: the case reads once more, in the batches the scans saw
    k = ksize
    written = 0
    case_reads = kevlar_amd.multi_file_iter_khmer([path for files in casefiles for path in files])
    batches = _after_skip(novel._batches(case_reads, ksize, k, batchsize), skipuntil)
    j = 0
    while True:
        text = None                 # this rank's batch j; None: it is at the end of the reads, or has failed
        if ranks.failure is None:
            try:
                text = next(batches, (None, 0))[0]
            except Exception as exc:
                ranks.fail(exc)
        if text is None and ranks.world == 1:
            break
        try:
            runs = [band_runs[j] for band_runs in per_band if j < len(band_runs)] if text is not None else []
            if text is not None and len(runs) != len(mine):
                ranks.fail(AllBandsFailed('the case reads have more batches than were scanned ({})'.format(j + 1)))
            lengths = [len(r[0]) for r in runs]
            d_rows = torch.from_numpy(_rows(runs, S)).to(device)
            if ranks.world > 1:
                # the end of the reads is agreed like everything else: a rank with a batch brings the lengths of its runs, a
                # rank at the end brings none; they are at the end together, for files and batch size are the same on all
                all_len, total_runs = ranks.gather(torch.tensor(lengths, dtype=torch.int64, device=device), len(lengths))
                if total_runs == 0:
                    break
                all_rows, _ = ranks.gather(d_rows, len(d_rows))
                if ranks.rank == 0:
                    per_rank = all_len.cpu().numpy().reshape(ranks.world, -1)
                    longest = all_rows.shape[0] // ranks.world
                    d_rows = torch.cat([all_rows[r * longest:r * longest + int(per_rank[r].sum())] for r in range(ranks.world)], dim=0)
                    lengths = [int(v) for r in range(ranks.world) for v in per_rank[r]]
            j += 1
            if text is None or ranks.rank != 0 or ranks.failure is not None or sum(lengths) == 0:
                continue
            try:
                hits = _merge(d_rows, lengths, S)
                blob = text.augmented_text(hits, k) if hasattr(text, 'augmented_text') else None
                if blob is None:
                    blob = ''.join(kevlar_amd.sequence.format_augmented_fastx(rec)
                                   for rec in novel._annotate(text, hits, k, novel._Tally())).encode('latin-1')
                written += int(np.count_nonzero(np.diff(hits[0]))) + 1
            except AllBandsFailed:
                raise
            except Exception as exc:
                ranks.fail(exc)
                continue
        finally:
            if text is not None:
                text.batch.close()
        if blob:
            yield blob
    if ranks.world > 1:
        # the closing gather: the bands' tallies meet on rank 0 -- and a rank that failed in the last batch says so here
        sums, _ = ranks.gather(torch.tensor([[instances, kmers]], dtype=torch.int64, device=device), 1)
        sums = sums.cpu().numpy().reshape(ranks.world, 2).sum(axis=0)
        instances, kmers = int(sums[0]), int(sums[1])
    if tally is not None:
        tally.update(instances=instances, kmers=kmers, reads=written)
    kevlar_amd.plog('[kevlar::novel]', 'Found {:d} instances of {:d} unique novel kmers in {:d} reads in {:.2f} seconds'.format(
        instances, kmers, written, clock.stop()))


def _check(args):
    """the combinations --all-bands does not take: refused before anything touches a device"""
    if getattr(args, 'distributed', False) and not getattr(args, 'all_bands', False):
        raise ValueError('--distributed shares the bands of an --all-bands run between the ranks: give --all-bands (and --num-bands)')
    if not args.num_bands:
        raise ValueError('--all-bands needs --num-bands N: the number of bands to run and merge')
    if args.num_bands < 1:
        raise ValueError('--num-bands must be at least 1')
    if args.band:
        raise ValueError('--all-bands runs every band: --band cannot be given with it')
    if args.case_counts or args.control_counts or args.save_case_counts or args.save_ctrl_counts:
        raise ValueError('--all-bands has N tables per sample: loading or saving count tables (--case-counts, --control-counts, '
                         '--save-case-counts, --save-ctrl-counts) is out of scope with it; save them band by band (--band I)')
    if getattr(args, 'ref_band_quirk', False):
        raise ValueError('--all-bands merges the hash-range bands of the banded count; the union of the literal low-bits bands of '
                         '--ref-band-quirk is not its result (SURVEY.md 0.4)')


def _join(backend):
    """torch first (its HIP runtime must be the one the process loads), this rank's device for torch and for the library,
    then the process group the environment describes (env://: torch reads RANK, WORLD_SIZE, MASTER_ADDR, MASTER_PORT)"""
    import torch
    torch.cuda.init()
    ndev = torch.cuda.device_count()
    index = int(os.environ.get('LOCAL_RANK', '0')) % max(1, ndev)
    os.environ['LOCAL_RANK'] = str(index)              # kevlar_amd._lib binds the library to the same device
    torch.cuda.set_device(index)
    _lib.require_device()
    if backend is False:
        return None
    import torch.distributed as dist
    if backend == 'nccl':
        dist.init_process_group('nccl', device_id=torch.device('cuda', index))
    elif backend == 'gloo':
        dist.init_process_group('gloo')
    else:
        # no choice made: both transports are set up (gloo for host tensors, RCCL for device tensors -- that one only when first
        # used) and the ranks take RCCL if each of them has a device of its own, else gloo, staged through the host (_Ranks)
        dist.init_process_group('cpu:gloo,cuda:nccl')
    world = dist.get_world_size()
    if world > MAX_RANKS:
        dist.destroy_process_group()
        raise ValueError('--distributed: {} ranks; at most {} ranks per node share the bands'.format(world, MAX_RANKS))
    return dist.group.WORLD


def main(args):
    _check(args)
    clock = kevlar_amd.Timer()
    clock.start()
    distributed = getattr(args, 'distributed', False)
    group = _join(getattr(args, 'dist_backend', None) if distributed else False)
    rank = 0
    if group is not None:
        import torch.distributed as dist
        rank = dist.get_rank(group)
    log = (kevlar_amd.logstream, kevlar_amd.teelog)
    if rank != 0:               # rank 0 speaks for the run
        kevlar_amd.logstream, kevlar_amd.teelog = open(os.devnull, 'w'), False
    sink = None
    try:
        for blob in novel_all_bands(args.case, args.control or [], args.ksize, args.memory, args.max_fpr, args.num_bands, args.case_min,
                                    args.ctrl_max, abundscreen=args.abund_screen, skipuntil=args.skip_until, numthreads=args.threads,
                                    group=group):
            if sink is None:
                sink = kevlar_amd.open_sink(args.out)
            sink.write(blob)
        if sink is None and rank == 0:
            sink = kevlar_amd.open_sink(args.out)       # nothing found: an empty file, as a per-band run leaves
        if sink is not None:
            sink.close()
    except BaseException:
        if sink is not None:            # a partly written output is worse than none
            sink.close()
            if args.out not in ('-', None) and os.path.exists(args.out):
                os.remove(args.out)
        raise
    finally:
        if rank != 0:
            kevlar_amd.logstream.close()
        kevlar_amd.logstream, kevlar_amd.teelog = log
        if group is not None:
            import torch.distributed as dist
            if dist.is_initialized():
                dist.destroy_process_group()
    kevlar_amd.plog('[kevlar::novel]', 'Total time: {:.2f} seconds'.format(clock.stop()))
