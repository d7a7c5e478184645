"""Host-side argument validation of the device rANS entry points (csrc/rans_device.hip): bad arguments come back
as TMAE_EINVAL (a ValueError with a message) before any launch, so this runs without a device.  CPU only."""
import ctypes

import pytest

LL = ctypes.c_longlong
D = 0x1000  # stands for a device address: validation never dereferences it


def enc_args(**kw):
    a = dict(symbols=D, sym_ss=0, sym_ts=8, indexes=D, idx_ss=0, idx_ts=8, nstreams=2, nseg=1, seg_len=8, cdfs=D,
             cdf_stride=4, cdf_sizes=D, offsets=D, ncdf=2, slabs=D, cap_words=16, nwords=D, status=D, stream=None)
    a.update(kw)
    return list(a.values())


def dec_args(**kw):
    a = dict(words=D, total_words=8, word_offsets=D, word_counts=D, indexes=D, idx_ss=0, idx_ts=8, symbols=D, sym_ss=0,
             sym_ts=8, nstreams=2, seg0=0, nseg=1, seg_len=8, cdfs=D, cdf_stride=4, cdf_sizes=D, offsets=D, ncdf=2,
             state=D, pos=D, status=D, first=1, stream=None)
    a.update(kw)
    return list(a.values())


def pack_args(**kw):
    a = dict(slabs=D, cap_words=16, nwords=D, nstreams=2, dense=D, dense_cap_words=32, word_offsets=D, status=D,
             stream=None)
    a.update(kw)
    return list(a.values())


@pytest.mark.parametrize("bad", [dict(symbols=None), dict(indexes=None), dict(slabs=None), dict(nwords=None),
                                 dict(status=None), dict(cdfs=None), dict(cdf_sizes=None), dict(offsets=None),
                                 dict(nstreams=0), dict(nstreams=-1), dict(seg_len=0), dict(nseg=0), dict(cdf_stride=1),
                                 dict(cap_words=0)])
def test_encode_streams_rejects(tmae, bad):
    from textmae_amd import _lib

    with pytest.raises(ValueError, match="tmae_rans_encode_streams: .+"):
        _lib.call("tmae_rans_encode_streams", *enc_args(**bad))


@pytest.mark.parametrize("bad", [dict(words=None), dict(word_offsets=None), dict(word_counts=None), dict(indexes=None),
                                 dict(symbols=None), dict(state=None), dict(pos=None), dict(status=None),
                                 dict(cdfs=None), dict(nstreams=0), dict(seg_len=0), dict(nseg=0), dict(cdf_stride=1),
                                 dict(seg0=-1)])
def test_decode_streams_rejects(tmae, bad):
    from textmae_amd import _lib

    with pytest.raises(ValueError, match="tmae_rans_decode_streams: .+"):
        _lib.call("tmae_rans_decode_streams", *dec_args(**bad))


@pytest.mark.parametrize("bad", [dict(slabs=None), dict(nwords=None), dict(dense=None), dict(word_offsets=None),
                                 dict(status=None), dict(nstreams=0), dict(cap_words=0)])
def test_pack_streams_rejects(tmae, bad):
    from textmae_amd import _lib

    with pytest.raises(ValueError, match="tmae_rans_pack_streams: .+"):
        _lib.call("tmae_rans_pack_streams", *pack_args(**bad))


def test_stream_capacity_bound(tmae):
    """ceil(52 n / 32) + n / 2^19 + 3 words: 52 = 16 + 4 (1 + 8) bits is the most one symbol adds"""
    from textmae_amd import ops

    assert ops.rans_stream_cap_words(0) == 3
    assert ops.rans_stream_cap_words(1) == 2 + 3
    assert ops.rans_stream_cap_words(333) == (52 * 333 + 31) // 32 + 3
    assert ops.rans_stream_cap_words(1 << 20) == 52 * (1 << 20) // 32 + 2 + 3
