"""Variant calls and their VCF text (the reference's kevlar/vcf.py): `Variant`, `VCFWriter`, `VCFReader`.

Everything here is host bookkeeping on whole strings; nothing walks a sequence.  The header and the records are the bytes the
reference prints (tests/golden/call/recorded.json holds them), so the descriptions below are its wording, typing slips
included."""
from collections import defaultdict
from datetime import date
from enum import Enum

from numpy import float64

import kevlar_amd


class VariantAnnotationError(ValueError):
    pass


class KevlarMixedDataTypeError(ValueError):
    pass


VariantFilter = Enum('VariantFilter', [
    'PerfectMatch', 'InscrutableCigar', 'PassengerVariant', 'PartitionScore', 'LikelihoodFail', 'NumerousMismatches', 'UserFilter',
    'ControlAbundance', 'CaseAbundance', 'Homopolymer', 'AmbiguousCall',
])


class FormattedList(list):
    """The values of one INFO key: '.' when empty, comma-separated otherwise, floats with three decimals.  Values of more than
    one type do not print."""

    def __str__(self):
        kinds = {type(value) for value in self}
        if not kinds:
            return '.'
        if len(kinds) > 1:
            raise KevlarMixedDataTypeError('mixed data type: ' + ','.join(sorted(str(kind) for kind in kinds)))
        if kinds & {float, float64}:
            return ','.join('{:.3f}'.format(value) for value in self)
        return ','.join(str(value) for value in self)


class Variant(object):
    """A call or a no-call ('.' for the alleles) at a 0-based position."""

    def __init__(self, seqid, pos, refr, alt, **kwargs):
        self._seqid, self._pos, self._refr, self._alt = seqid, pos, refr, alt
        self._filters = set()
        self.info = defaultdict(FormattedList)
        for key, value in kwargs.items():
            self.annotate(key, value)
        self._sample_data = defaultdict(dict)

    def __str__(self):
        if len(self._refr) == 1 and len(self._alt) == 1:
            return '{:s}:{:d}:{:s}->{:s}'.format(self._seqid, self._pos, self._refr, self._alt)
        if len(self._refr) > len(self._alt):
            return '{:s}:{:d}:{:d}D'.format(self._seqid, self._pos + 1, len(self._refr) - len(self._alt))
        return '{:s}:{:d}:I->{:s}'.format(self._seqid, self._pos + 1, self._alt[1:])

    def format(self, sample, key, value_to_store=None):
        """the FORMAT value of a sample: stored when one is given, else returned (None when there is none)"""
        if value_to_store is not None:
            self._sample_data[sample][key] = value_to_store
            return None
        return self._sample_data[sample].get(key) if sample in self._sample_data else None

    @property
    def seqid(self):
        return self._seqid

    @property
    def position(self):
        return self._pos

    @property
    def region(self):
        return self._seqid, self._pos, self._pos + len(self._refr)

    @property
    def vcf(self):
        """the eight fixed columns; INFO keys in order, CONTIG last"""
        info = '.'
        if self.info:
            pairs = [self.attribute(key, pair=True) for key in sorted(self.info) if key != 'CONTIG']
            contig = self.attribute('CONTIG', pair=True)
            if contig:
                pairs.append(contig)
            info = ';'.join(pairs)
        pos = self._pos if self._pos == '.' else self._pos + 1
        return '{:s}\t{}\t.\t{:s}\t{:s}\t.\t{:s}\t{:s}'.format(self._seqid, pos, self._refr, self._alt, self.filterstr, info)

    @property
    def cigar(self):
        return self.attribute('CIGAR')

    @property
    def window(self):
        """the stretch of the contig that holds every k-mer overlapping the alternate allele"""
        return self.attribute('ALTWINDOW')

    @property
    def windowlength(self):
        window = self.window
        return 0 if window is None else len(window)

    @property
    def refrwindow(self):
        """the same stretch of the reference"""
        return self.attribute('REFRWINDOW')

    def annotate(self, key, value, replace=True):
        if replace:
            self.info[key] = FormattedList([value])
        else:
            self.info[key].append(value)

    def attribute(self, key, pair=False, string=False):
        """The value of an INFO key (None when absent): as it was stored (the list when there are several), as a string, or as
        the `KEY=values` pair of the INFO column."""
        if key not in self.info:
            return None
        values = self.info[key]
        if pair:
            return '{:s}={:s}'.format(key, str(values))
        if string:
            return str(values)
        return values[0] if len(values) == 1 else values

    def filter(self, filtertype):
        if isinstance(filtertype, VariantFilter):
            self._filters.add(filtertype)

    @property
    def filterstr(self):
        if self._filters:
            return ';'.join(sorted(kind.name for kind in self._filters))
        return '.' if self._refr == '.' else 'PASS'

    @property
    def genotypes(self):
        found = self.attribute('GT')
        return tuple(found.split(',')) if found else None

    def test_merge(self, other):
        """This substitution extended by `other` when that is the substitution right behind it on the same contig (their
        windows overlap as neighbours' do); None when the two do not merge."""
        if self.seqid == '.' or self.seqid != other.seqid:
            return None
        if len(self._alt) != len(self._refr) or len(other._alt) != len(other._refr):
            return None
        length = len(self._refr)
        if self.position != other.position - length:
            return None
        if None in (self.window, other.window, self.refrwindow, other.refrwindow):
            return None
        if self.window[length:] != other.window[:-1] or self.refrwindow[length:] != other.refrwindow[:-1]:
            return None
        # (the windows become plain strings here, as in the reference)
        self.info['ALTWINDOW'] = self.window + other.window[-length]
        self.info['REFRWINDOW'] = self.refrwindow + other.refrwindow[-length]
        self._alt += other._alt
        self._refr += other._refr
        return self


class VCFWriter(object):
    filter_desc = {
        VariantFilter.PerfectMatch: 'No mismatches between contig with putatively novel content and reference target',
        VariantFilter.InscrutableCigar: 'Alignment path/structure cannot be interpreted as a variant',
        VariantFilter.PassengerVariant: 'A mismatch between contig and reference that is not spanned by any novel k-mers',
        VariantFilter.PartitionScore: 'Expectation is 1 variant call per partition, so all call(s) with suboptimal likelihood '
                                      'scores are filtered',
        VariantFilter.LikelihoodFail: 'Variant calls with a likelihood score < 0.0 are unlikely to bereal',
        VariantFilter.NumerousMismatches: 'No attempt at variant calling was made due to a suspicious number of mismatches '
                                          'between the contig and the reference genome',
        VariantFilter.UserFilter: 'The user has explicitly filtered this variant out due to overlap with problematic/undesired '
                                  'loci or variants.',
        VariantFilter.ControlAbundance: 'Too many variant-spanning k-mers have high abundance in one or more control samples.',
        VariantFilter.CaseAbundance: 'Too many consecutive variant-spanning k-mers have low abundance in the case/proband sample.',
        VariantFilter.Homopolymer: 'Indels associate with homopolymers are most often spurious and very difficult to verify with '
                                   'confidence.',
        VariantFilter.AmbiguousCall: 'Derived from a contig with too many distinct, equally optimal variant calls.',
    }

    # label: (type, number, description), in the order they are printed
    info_metadata = {
        'ALTWINDOW': ('String', '1', 'window containing all k-mers that span the variant alternate allele'),
        'CIGAR': ('String', '1', 'alignment path'),
        'IKMERS': ('Integer', '1', 'number of "interesting" (novel) k-mers spanning the variant alternate allele'),
        'KSW2': ('Float', '1', 'alignment score'),
        'REFRWINDOW': ('String', '1', 'window containing all k-mers that span the variant reference allele'),
        'REFRCOPYNUM': ('Integer', '.', 'number of times each reference allele k-mer occurs in the reference genome'),
        'CONTIG': ('String', '1', 'contig assembled from reads containing novel k-mers, aligned to reference to call variants'),
        'LIKESCORE': ('Float', '1', 'likelihood score of the variant, computed as `LLDN - max(LLIH, LLFP)`'),
        'LLDN': ('Float', '1', 'log likelihood that the variant is a de novo variant'),
        'LLIH': ('Float', '1', 'log likelihood that the variant is an inherited variant'),
        'LLFP': ('Float', '1', 'log likelihood that the variant is a false call'),
        'DROPPED': ('Integer', '1', 'number of k-mers dropped from ALTWINDOW for likelihood calculations because it is present '
                                    'elsewhere in the genome (not novel)'),
    }

    format_metadata = {
        'ALTABUND': ('Integer', '.', 'abundance of alternate allele k-mers'),
    }

    def __init__(self, outstream, source='kevlar', refr=None):
        self._out = outstream
        self._sample_labels = []
        self._source = source
        self._refr = refr
        self.format_metadata = dict(type(self).format_metadata)       # describe_format is this writer's (the reference's is the class's)

    def register_sample(self, label):
        self._sample_labels.append(label)

    def register_samples_from_reader(self, reader):
        for label in reader._sample_labels:
            self.register_sample(label)

    def describe_format(self, label, datatype, datanumber, desc):
        self.format_metadata[label] = (datatype, datanumber, desc)

    def header_lines(self, skipdate=False):
        lines = ['##fileformat=VCFv4.2']
        if not skipdate:
            lines.append('##fileDate=' + date.today().isoformat())
        if self._source:
            lines.append('##source=' + self._source)
        if self._refr:
            lines.append('##reference=' + self._refr)
        lines.extend('##FILTER=<ID={},Description="{}">'.format(kind.name, self.filter_desc[kind]) for kind in VariantFilter)
        for tag, table in (('INFO', self.info_metadata), ('FORMAT', self.format_metadata)):
            for label, (datatype, number, desc) in table.items():
                lines.append('##{}=<ID={},Number={},Type={},Description="{}">'.format(tag, label, number, datatype, desc))
        columns = ['CHROM', 'POS', 'ID', 'REF', 'ALT', 'QUAL', 'FILTER', 'INFO']
        if self._sample_labels:
            columns += ['FORMAT'] + self._sample_labels
        lines.append('#' + '\t'.join(columns))
        return lines

    def write_header(self, skipdate=False):
        self._out.write(''.join(line + '\n' for line in self.header_lines(skipdate)))

    def record_line(self, variant):
        """the variant's line: its fixed columns, then FORMAT and one column per registered sample"""
        keys_seen, columns = None, []
        for sample in self._sample_labels:
            pairs = [(field, variant.format(sample, field)) for field in sorted(self.format_metadata)]
            pairs = [(field, value) for field, value in pairs if value]
            keys = ':'.join(field for field, value in pairs)
            if keys_seen is None:
                keys_seen = keys
            elif keys != keys_seen:
                raise VariantAnnotationError('samples not annotated with the same FORMAT fields ({:s} vs {:s})'.format(keys_seen, keys))
            columns.append(':'.join(value for field, value in pairs))
        if not columns:
            return variant.vcf
        return '\t'.join([variant.vcf, keys_seen] + columns)

    def write(self, variant):
        self._out.write(self.record_line(variant) + '\n')


class VCFReader(object):
    def __init__(self, instream):
        self._in = instream
        self._sample_labels = []
        self.suppress_filter_warnings = False

    def _variant_from_vcf_string(self, vcfstr):
        fields = vcfstr.strip().split('\t')
        pos = '.' if fields[1] == '.' else int(fields[1]) - 1
        variant = Variant(fields[0], pos, fields[3], fields[4])
        for item in fields[7].split(';'):
            if '=' in item:
                key, values = item.split('=')
                for value in values.split(','):
                    variant.annotate(key, value)           # (replacing: of several values the last one stays, as in the reference)
            else:
                variant.annotate(item, True)
        if fields[6] not in ('.', 'PASS'):
            for label in fields[6].split(';'):
                if label in VariantFilter.__members__:
                    variant.filter(VariantFilter[label])
                elif not self.suppress_filter_warnings:
                    kevlar_amd.plog('[kevlar::vcf]', 'filter "{}" not recognized; attempting to write this variant to VCF will '
                                                     'probably turn out poorly'.format(fields[6]))
        if len(fields) > 9:
            keys, samples = fields[8].split(':'), fields[9:]
            if self._sample_labels and len(samples) != len(self._sample_labels):
                raise VariantAnnotationError('sample number mismatch: ' + vcfstr)
            for label, data in zip(self._sample_labels, samples):
                if data in ('.', './.'):
                    continue
                values = data.split(':')
                if len(keys) != len(values):
                    raise VariantAnnotationError('format data mismatch: ' + vcfstr)
                for key, value in zip(keys, values):
                    variant.format(label, key, value)
        return variant

    def __iter__(self):
        for line in self._in:
            if not line.startswith('#'):
                kevlar_amd.plog('[kevlar::vcf]', 'WARNING: VCF file has no samples annotated, certain sanity checks disabled')
                yield self._variant_from_vcf_string(line)
                break
            if line.startswith('#CHROM\t'):
                self._save_samples(line)
                break
        for line in self._in:
            if not line.startswith('#'):
                yield self._variant_from_vcf_string(line)

    def _save_samples(self, line):
        fields = line.strip().split('\t')
        assert len(fields) >= 8
        if len(fields) > 8:
            self._sample_labels = fields[9:]


def vcfstream(filelist):
    for infile in filelist:
        for record in VCFReader(kevlar_amd.open(infile, 'r')):
            yield record
