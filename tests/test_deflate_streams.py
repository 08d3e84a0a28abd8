"""tests/deflate_common.py against zlib's inflate on the host: every stream of the catalogue that is to be accepted inflates to
exactly the text its tokens mean (two references that owe each other nothing), every one that is to be refused is refused with
the recorded message.  This proves the assembler and pins the reference's verdict before any device is involved
(tests/test_gpu_deflate.py runs the same catalogue through the two device inflaters)."""
import gzip
import zlib

import pytest

import deflate_common as dc


def test_the_catalogue_has_every_group():
    for name in dc.GROUPS + ['rejected']:
        assert dc.group(name), name
    assert len(dc.group('tables')) == 31 and len(dc.group('rejected')) >= 25
    assert {c[0] for c in dc.group('rejected')} == set(dc.LENIENT)


@pytest.mark.parametrize('name', dc.GROUPS)
def test_zlib_inflates_the_accepted_streams_to_the_text_their_tokens_mean(name):
    for case, raw, text in dc.group(name):
        assert isinstance(text, bytes), case
        assert dc.reference(raw) == text, case
        if dc.fits_bgzf(raw, text):
            assert gzip.decompress(dc.bgzf_member(raw, text) + dc.BGZF_EOF) == text, case
        assert gzip.decompress(dc.gzip_member(raw, text, flags=2 | 8)) == text, case


def test_zlib_refuses_the_rejected_streams_with_the_recorded_message():
    for case, raw, message in dc.group('rejected'):
        assert isinstance(message, str), case
        with pytest.raises(zlib.error) as err:
            dc.reference(raw)
        assert str(err.value).endswith(': ' + message), (case, str(err.value))
        # ... framed as a file too, behind a trailer that announces what a decoder that missed the fault would produce
        with pytest.raises(zlib.error):
            gzip.decompress(dc.gzip_member(raw, dc.LENIENT[case]))


def test_the_longest_codes_of_the_staircases_are_longer_than_the_decoders_tables():
    """kv_gunzip.hip looks 9 bits of a literal/length code up, kv_inflate.hip 10, both 8 of a distance code: the deep cases
    must go beyond all of them"""
    assert max(dc.staircase(16, range(16))) == 15 and sorted(dc.staircase(16, range(16)))[:11] == list(range(1, 12))


def test_whole_files_inflate_to_their_text_or_are_refused():
    for case, image, text in dc.IMAGES:
        if text is None:
            with pytest.raises((OSError, zlib.error, EOFError)):
                gzip.decompress(image)
        else:
            assert gzip.decompress(image) == text, case


@pytest.mark.parametrize('strategy', sorted(dc.STRATEGIES))
def test_zlib_space_round_trips(strategy):
    cases = dc.zlib_space(strategy)
    assert len(cases) == 18
    for case, raw, text in cases:
        assert dc.reference(raw) == text, case
