"""Self-contained per-image bitstream, container version 1 (DESIGN.md "Container format"): the host part.

One blob per image carries everything ``MCM.decode_bytes`` needs.  Little-endian, a whole number of 32-bit words:

    bytes 0-3    b"TMC" + version byte 1
          4-5    img_size u16
          6-7    num_keep_patches K u16
          8      patch_size u8
          9      low nibble log2(lanes), high nibble log2(z_lanes)
          10-11  length of the z record in 32-bit words, u16
          12-13  original width u16, 14-15 original height u16 (0, 0 = not recorded)
          then   W = ceil(K * bits / 32) words of kept ids
          then   the z record, then the y record (the rest of the blob)

L = (img_size / patch_size)^2 and bits = max(1, ceil(log2 L)).  Id k (= ids_shuffle[k], the patch token k came
from) occupies bits [k * bits, (k + 1) * bits) of the id section's bit string, LSB first; bit i of the string is
bit i % 32 of word i / 32; unused tail bits are zero.  The records are the strings ``MCM.compress_batch`` returns:
the plain rANS stream at one lane, the ``coder.encode_record`` record at more.

``pack_ids_host`` / ``unpack_ids_host`` restate the two device kernels (csrc/ids_pack.hip) in numpy; the tests use
them as the oracle.  Nothing here touches the device.

A second format, b"TMT" version 1 (``assemble_image`` / ``parse_image`` / ``tile_blob``, layout further down), holds
one image coded at its own resolution as overlapping tiles: the sections of the tiles' TMC blobs behind one header
and a table of record lengths (``MCM.encode_image`` / ``decode_image``).  ``read_image_index`` /
``read_tiles`` read such a file's header and table and then single tiles, from bytes or from a file object, without
touching the other tiles (``MCM.decode_region`` / ``decode_crops``).

Blobs and files whose y latents were coded at a quantiser step other than 1 (``q=`` of the model's methods, DESIGN.md
§3.17) carry the magics b"TQC" / b"TQT" and the ladder position q; every reader here takes both kinds and returns q
as the last field of its tuple (0 for TMC / TMT).  ``qstep`` is the ladder.

Blobs and files coded with a quantiser step per kept patch (``qoffsets=``) carry the magics b"TPC" /
b"TPT": a base position q, a table of nlev ladder offsets and per kept patch a level into that table, packed like the
ids.  The readers return them as trailing fields (nlev, offsets, level words), nlev = 1 and no level words for the other
magics.  ``select_levels_host`` / ``pack_levels_host`` / ``unpack_levels_host`` / ``build_qmap_host`` at the end restate
the kernels of csrc/qlevels.hip in numpy.
"""
from __future__ import annotations

import struct
from typing import NamedTuple

import numpy as np

MAGIC = b"TMC"
VERSION = 1
HEADER_BYTES = 16
# the same blob coded at a quantiser step other than 1: the 16 TMC header bytes, then one word
# holding the ladder position q as int8 and three zero bytes, then ids, z and y as in TMC.  q = 0 is always TMC.
QMAGIC = b"TQC"
QHEADER_BYTES = 20
Q_MIN, Q_MAX = -32, 32
# F[k] = the f32 nearest to 2^(k/8), the literals of tmae_qstep (csrc/common.h)
QSTEP_F = (1.0, 1.09050775, 1.18920708, 1.29683959, 1.41421354, 1.54221082, 1.68179286, 1.8340081)
# the same blob with a quantiser step per kept patch: the 16 TMC header bytes; one word holding the
# base position q as int8 (0 allowed), the table size nlev (2..16) and two zero bytes; 16 bytes of int8 ladder offsets
# (-64..64, entries at index >= nlev zero); the id words; W2 = level_words(K, nlev) level words (level of kept patch k
# at bits [k * lbits, (k + 1) * lbits), lbits = level_bits(nlev), the ids' bit order); then z and y as in TMC.
PMAGIC = b"TPC"
PHEADER_BYTES = 36
NLEV_MIN, NLEV_MAX = 2, 16
OFFSET_MIN, OFFSET_MAX = -64, 64
MAX_L = 1024       # IDS_MAXL of the kernels
MAX_LANE_LOG2 = 6  # lanes <= 64 (coder.check_lanes)
_HEADER = struct.Struct("<3sBHHBBHHH")

# status words of unpack (tmae_ids_unpack)
IDS_STATUS = {1: "patch id outside the image", 2: "duplicate patch id", 3: "non-zero padding bits"}


def check_q(q, who="q") -> int:
    """q as an int in Q_MIN..Q_MAX, ValueError otherwise"""
    v = int(q)
    if v != q or not Q_MIN <= v <= Q_MAX:
        raise ValueError(f"{who} = {q!r} outside {Q_MIN}..{Q_MAX} (integer positions on the quantiser step ladder)")
    return v


def qstep(q) -> np.float32:
    """the quantiser step of ladder position q: F[q mod 8] * 2^floor(q / 8) as f32, 1/16 .. 16, qstep(0) = 1; the
    mirror of tmae_qstep (csrc/common.h), which the kernels evaluate themselves"""
    v = check_q(q)
    return np.ldexp(np.float32(QSTEP_F[v % 8]), v // 8).astype(np.float32)


def _read_q(byte, what, plain):
    """the int8 ladder position of a TQC / TQT header: never 0 (that is written as `plain`), within the ladder"""
    q = byte - 256 if byte >= 128 else byte
    if q == 0:
        raise ValueError(f"{what} stream with q = 0: a step of 1 is written as {plain}")
    if not Q_MIN <= q <= Q_MAX:
        raise ValueError(f"{what} stream with q = {q}: the ladder is {Q_MIN}..{Q_MAX}")
    return q


# status words of tmae_qlevels_unpack / tmae_qlevels_select
LEVELS_STATUS = {1: "quantiser level outside its table", 2: "non-zero padding bits of the level section"}


def level_bits(nlev: int) -> int:
    """bits of one packed level: max(1, ceil(log2 nlev))"""
    return max(1, (int(nlev) - 1).bit_length())


def level_words(K: int, nlev: int) -> int:
    """32-bit words of the level section: ceil(K * lbits / 32); none for nlev = 1 (no map)"""
    return 0 if int(nlev) < 2 else (int(K) * level_bits(nlev) + 31) // 32


def check_offsets(offsets, who="qoffsets") -> tuple:
    """the table of ladder offsets as a tuple of nlev ints: 2..16 integers in -64..64, ValueError otherwise"""
    try:
        offs = list(offsets.tolist() if hasattr(offsets, "tolist") else offsets)
    except TypeError:
        raise ValueError(f"{who} = {offsets!r}: a sequence of {NLEV_MIN}..{NLEV_MAX} integers") from None
    if not NLEV_MIN <= len(offs) <= NLEV_MAX:
        raise ValueError(f"{who}: nlev = {len(offs)} outside {NLEV_MIN}..{NLEV_MAX} (the entries of the offset table)")
    out = []
    for i, o in enumerate(offs):
        v = int(o)
        if v != o or not OFFSET_MIN <= v <= OFFSET_MAX:
            raise ValueError(f"{who}[{i}] = {o!r}: offset outside {OFFSET_MIN}..{OFFSET_MAX} (integers)")
        out.append(v)
    return tuple(out)


def _offset_bytes(offsets) -> bytes:
    """the 16 int8 bytes of the offset table, entries past nlev zero"""
    return struct.pack("<16b", *(tuple(offsets) + (0,) * (NLEV_MAX - len(offsets))))


def _read_table(qbyte, nlev, table, what):
    """q, nlev and the 16 offset bytes of a TPC / TPT header -> (q, offsets tuple of nlev ints)"""
    q = qbyte - 256 if qbyte >= 128 else qbyte
    if not Q_MIN <= q <= Q_MAX:
        raise ValueError(f"{what} stream with q = {q}: the ladder is {Q_MIN}..{Q_MAX}")
    if not NLEV_MIN <= nlev <= NLEV_MAX:
        raise ValueError(f"{what} stream with nlev = {nlev}: outside {NLEV_MIN}..{NLEV_MAX}")
    offs = struct.unpack("<16b", bytes(table))
    for i, o in enumerate(offs[:nlev]):
        if not OFFSET_MIN <= o <= OFFSET_MAX:
            raise ValueError(f"{what} stream: offset {i} = {o} outside {OFFSET_MIN}..{OFFSET_MAX}")
    if any(offs[nlev:]):
        raise ValueError(f"{what} stream: unused offsets {offs[nlev:]} past nlev = {nlev} must be zero")
    return q, offs[:nlev]


class Blob(NamedTuple):
    """parse()'s result: the header fields, then views of the three sections"""
    img_size: int
    num_keep_patches: int
    patch_size: int
    lanes: int
    z_lanes: int
    orig_size: tuple | None  # (width, height) or None when not recorded
    ids: np.ndarray          # uint32 [W] view
    z: memoryview
    y: memoryview
    q: int = 0               # ladder position of the y quantiser step (0: a TMC blob, else a TQC one; TPC: the base)
    nlev: int = 1            # TPC: entries of the offset table (1: no map, the other magics)
    offsets: tuple = ()      # TPC: the nlev ladder offsets
    levels: np.ndarray | None = None  # TPC: uint32 [W2] view of the level words

    @property
    def num_patches(self) -> int:
        return (self.img_size // self.patch_size) ** 2


def id_bits(L: int) -> int:
    """bits of one packed id: max(1, ceil(log2 L))"""
    return max(1, (int(L) - 1).bit_length())


def id_words(L: int, K: int) -> int:
    """32-bit words of the id section: ceil(K * bits / 32)"""
    return (int(K) * id_bits(L) + 31) // 32


def _log2_lanes(lanes, name):
    v = int(lanes)
    if v < 1 or v & (v - 1) or v > 1 << MAX_LANE_LOG2:
        raise ValueError(f"{name} = {lanes!r} must be a power of two in 1..{1 << MAX_LANE_LOG2}")
    return v.bit_length() - 1


def _check_geometry(img_size, K, patch):
    if patch < 1 or img_size < 1 or img_size % patch:
        raise ValueError(f"patch_size {patch} does not divide img_size {img_size}")
    L = (img_size // patch) ** 2
    if L > MAX_L:
        raise ValueError(f"{L} patches: the format holds at most {MAX_L}")
    if not 1 <= K <= L:
        raise ValueError(f"num_keep_patches {K} outside 1..{L} (the number of patches)")
    return L


def pack_header(img_size, num_keep_patches, patch_size, lanes=1, z_lanes=1, z_words=0, orig_size=None, q=0,
                offsets=None) -> bytes:
    """the 16 header bytes (q = 0, TMC), the 20 of a TQC blob or, with a table of offsets, the 36 of a TPC blob;
    z_words = length of the z record in 32-bit words, orig_size = (width, height) or None"""
    q = check_q(q)
    if offsets is not None:
        offsets = check_offsets(offsets, "offsets")
    img_size, K, patch, z_words = int(img_size), int(num_keep_patches), int(patch_size), int(z_words)
    if not (0 < img_size < 1 << 16 and 0 < patch < 1 << 8):
        raise ValueError(f"img_size {img_size} / patch_size {patch} do not fit the header (u16 / u8)")
    _check_geometry(img_size, K, patch)
    if not 0 <= z_words < 1 << 16:
        raise ValueError(f"z record of {z_words} words does not fit the header's u16")
    w, h = (0, 0) if orig_size is None else (int(orig_size[0]), int(orig_size[1]))
    if not (0 <= w < 1 << 16 and 0 <= h < 1 << 16):
        raise ValueError(f"original size {(w, h)} does not fit the header's u16 fields")
    nib = _log2_lanes(lanes, "lanes") | _log2_lanes(z_lanes, "z_lanes") << 4
    if offsets is not None:
        return _HEADER.pack(PMAGIC, VERSION, img_size, K, patch, nib, z_words, w, h) \
            + struct.pack("<bBxx", q, len(offsets)) + _offset_bytes(offsets)
    if q:
        return _HEADER.pack(QMAGIC, VERSION, img_size, K, patch, nib, z_words, w, h) + struct.pack("<bxxx", q)
    return _HEADER.pack(MAGIC, VERSION, img_size, K, patch, nib, z_words, w, h)


def assemble(img_size, num_keep_patches, patch_size, lanes, z_lanes, orig_size, ids_words, z_record, y_record,
             q=0, offsets=None, level_words_=None) -> bytes:
    """one blob from its parts; ids_words: uint32-compatible [W] array (pack_ids_host / ops.ids_pack of one image);
    q: the ladder position the y record was coded at (0: a TMC blob, byte for byte; else TQC).  offsets (2..16 ints)
    and level_words_ (uint32-compatible [W2], pack_levels_host / ops.qlevels_pack of the image): a TPC blob, q its
    base position"""
    L = _check_geometry(int(img_size), int(num_keep_patches), int(patch_size))
    ids = np.ascontiguousarray(ids_words).view(np.uint32).reshape(-1).astype("<u4", copy=False)
    if ids.size != id_words(L, num_keep_patches):
        raise ValueError(f"{ids.size} id words, {id_words(L, num_keep_patches)} expected")
    z, y = bytes(z_record), bytes(y_record)
    if len(z) % 4 or len(y) % 4:
        raise ValueError(f"records are whole 32-bit words (z {len(z)} bytes, y {len(y)} bytes)")
    lev = b""
    if (offsets is None) != (level_words_ is None):
        raise ValueError("assemble: offsets and level words go together")
    if offsets is not None:
        offsets = check_offsets(offsets, "offsets")
        lv = np.ascontiguousarray(level_words_).view(np.uint32).reshape(-1).astype("<u4", copy=False)
        if lv.size != level_words(num_keep_patches, len(offsets)):
            raise ValueError(f"{lv.size} level words, {level_words(num_keep_patches, len(offsets))} expected")
        lev = lv.tobytes()
    return pack_header(img_size, num_keep_patches, patch_size, lanes, z_lanes, len(z) // 4, orig_size, q, offsets) \
        + ids.tobytes() + lev + z + y


def parse(blob) -> Blob:
    """header fields and views of the id words, the z record and the y record; ValueError on a blob that is not a
    well-formed version-1 TMC, TQC or TPC container (the records themselves are checked by the coder)"""
    mv = memoryview(blob).cast("B") if not isinstance(blob, memoryview) else blob.cast("B")
    n = len(mv)
    if n < HEADER_BYTES:
        raise ValueError(f"{n} bytes: shorter than the {HEADER_BYTES}-byte header")
    magic, version, img_size, K, patch, nib, z_words, w, h = _HEADER.unpack_from(mv, 0)
    if magic not in (MAGIC, QMAGIC, PMAGIC):
        raise ValueError(f"not a TMC bitstream (magic {bytes(magic)!r})")
    if version != VERSION:
        raise ValueError(f"container version {version}, this reader knows version {VERSION}")
    if n % 4:
        raise ValueError(f"{n} bytes: not a whole number of 32-bit words")
    q, hb = 0, HEADER_BYTES
    if magic == QMAGIC:
        hb = QHEADER_BYTES
        if n < hb:
            raise ValueError(f"{n} bytes: shorter than the {hb}-byte TQC header")
        q = _read_q(mv[16], "TQC", "TMC")
        if mv[17] or mv[18] or mv[19]:
            raise ValueError(f"TQC stream: padding bytes 17-19 hold {bytes(mv[17:20]).hex()}, must be zero")
    nlev, offsets = 1, ()
    if magic == PMAGIC:
        hb = PHEADER_BYTES
        if n < hb:
            raise ValueError(f"{n} bytes: shorter than the {hb}-byte TPC header")
        if mv[18] or mv[19]:
            raise ValueError(f"TPC stream: padding bytes 18-19 hold {bytes(mv[18:20]).hex()}, must be zero")
        q, offsets = _read_table(mv[16], mv[17], mv[20:36], "TPC")
        nlev = len(offsets)
    ll, zl = nib & 15, nib >> 4
    if ll > MAX_LANE_LOG2 or zl > MAX_LANE_LOG2:
        raise ValueError(f"lane fields 2^{ll} / 2^{zl}: at most 2^{MAX_LANE_LOG2} lanes")
    L = _check_geometry(img_size, K, patch)
    W, W2 = id_words(L, K), level_words(K, nlev)
    need = hb + 4 * (W + W2 + z_words + 2)
    if n < need:
        raise ValueError(f"{n} bytes: header + {W} id words + " + (f"{W2} level words + " if nlev > 1 else "")
                         + f"{z_words} z words + at least 2 y words take {need}")
    z0 = hb + 4 * (W + W2)
    y0 = z0 + 4 * z_words
    ids = np.frombuffer(mv, dtype="<u4", count=W, offset=hb)
    levels = np.frombuffer(mv, dtype="<u4", count=W2, offset=hb + 4 * W) if nlev > 1 else None
    return Blob(img_size, K, patch, 1 << ll, 1 << zl, (w, h) if (w, h) != (0, 0) else None, ids, mv[z0:y0], mv[y0:],
                q, nlev, offsets, levels)


# ------------------------------------------------------------------------------------ tiled images: b"TMT", version 1
# One file per image coded at its own resolution as overlapping model-sized tiles (tiling.py).
# Little-endian, a whole number of 32-bit words:
#
#     bytes 0-3    b"TMT" + version byte 1
#           4-5    tile size S u16, 6-7 K u16, 8 patch_size u8, 9 lane nibbles (all as in TMC)
#           10-11  overlap O u16
#           12-13  image width u16, 14-15 image height u16 (both >= 1)
#           16-17  chunk u16: the tile batch the encoder used (>= 1)
#           18-19  zero
#           20-23  T u32 = nx * ny of the fields above
#           then   T table entries: z_words u32, y_words u32
#           then   per tile, in order: W = id_words(L, K) id words, the z record, the y record
#
# b"TQT", version 1: the same file coded at one quantiser step other than 1: byte 18 holds the ladder
# position q as int8, byte 19 stays zero, everything else as above.  q = 0 is always TMT.
#
# b"TPT", version 1: the file coded with a quantiser step per kept patch: byte 18 holds the base
# position q as int8 (0 allowed), byte 19 the table size nlev (2..16); 16 bytes of int8 ladder offsets follow the 24
# header bytes (entries at index >= nlev zero), then the table; per tile the id words, W2 = level_words(K, nlev) level
# words, the z record and the y record.  One table of offsets per file, one level section per tile.
IMAGE_MAGIC = b"TMT"
IMAGE_QMAGIC = b"TQT"
IMAGE_PMAGIC = b"TPT"
IMAGE_PHEADER_BYTES = 40
IMAGE_VERSION = 1
IMAGE_HEADER_BYTES = 24
_IMAGE_HEADER = struct.Struct("<3sBHHBBHHHHHI")


class ImageBlob(NamedTuple):
    """parse_image()'s result: the header fields, then per tile views of the id words, the z and the y record"""
    img_size: int            # the tile size S
    num_keep_patches: int
    patch_size: int
    lanes: int
    z_lanes: int
    overlap: int
    width: int
    height: int
    chunk: int
    ids: list                # T uint32 [W] views
    z: list                  # T memoryviews
    y: list
    q: int = 0               # ladder position of the y quantiser step of every tile (0: a TMT file, else TQT; TPT: base)
    nlev: int = 1            # TPT: entries of the offset table (1: no map, the other magics)
    offsets: tuple = ()      # TPT: the nlev ladder offsets of the file
    levels: list | None = None  # TPT: T uint32 [W2] views of the tiles' level words

    @property
    def num_patches(self) -> int:
        return (self.img_size // self.patch_size) ** 2

    @property
    def num_tiles(self) -> int:
        return len(self.ids)


def assemble_image(img_size, num_keep_patches, patch_size, lanes, z_lanes, overlap, width, height, chunk, ids_words,
                   z_records, y_records, q=0, offsets=None, level_words_=None) -> bytes:
    """one TMT file from its parts; ids_words: uint32-compatible [T, W] (ops.ids_pack of the tiles), z_records /
    y_records: T byte strings each (compress_batch's records of the tiles, in tile order); q: the ladder position
    all tiles were coded at (0: a TMT file, byte for byte; else TQT).  offsets (2..16 ints) and level_words_
    (uint32-compatible [T, W2], ops.qlevels_pack of the tiles): a TPT file, q its base position"""
    from .tiling import grid

    q = check_q(q)
    if (offsets is None) != (level_words_ is None):
        raise ValueError("assemble_image: offsets and level words go together")
    if offsets is not None:
        offsets = check_offsets(offsets, "offsets")

    img_size, K, patch = int(img_size), int(num_keep_patches), int(patch_size)
    overlap, width, height, chunk = int(overlap), int(width), int(height), int(chunk)
    if not (0 < img_size < 1 << 16 and 0 < patch < 1 << 8):
        raise ValueError(f"img_size {img_size} / patch_size {patch} do not fit the header (u16 / u8)")
    L = _check_geometry(img_size, K, patch)
    if not (1 <= width < 1 << 16 and 1 <= height < 1 << 16):
        raise ValueError(f"image size {(width, height)} does not fit the header's u16 fields (both >= 1)")
    if not 1 <= chunk < 1 << 16:
        raise ValueError(f"chunk {chunk} outside 1..65535")
    g = grid(height, width, img_size, overlap)
    W = id_words(L, K)
    ids = np.ascontiguousarray(ids_words).view(np.uint32).reshape(-1, W).astype("<u4", copy=False)
    if not ids.shape[0] == len(z_records) == len(y_records) == g.T:
        raise ValueError(f"{ids.shape[0]} id rows, {len(z_records)} z and {len(y_records)} y records for {g.T} tiles")
    lev = None
    if offsets is not None:
        W2 = level_words(K, len(offsets))
        lev = np.ascontiguousarray(level_words_).view(np.uint32).reshape(-1, W2).astype("<u4", copy=False)
        if lev.shape[0] != g.T:
            raise ValueError(f"{lev.shape[0]} rows of level words for {g.T} tiles")
    table, body = [], []
    for t in range(g.T):
        z, y = bytes(z_records[t]), bytes(y_records[t])
        if len(z) % 4 or len(y) % 4 or len(z) < 8 or len(y) < 8:
            raise ValueError(f"tile {t}: records are whole 32-bit words, at least 2 (z {len(z)} bytes, y {len(y)} "
                             f"bytes)")
        table.append(struct.pack("<II", len(z) // 4, len(y) // 4))
        body += [ids[t].tobytes(), z, y] if lev is None else [ids[t].tobytes(), lev[t].tobytes(), z, y]
    nib = _log2_lanes(lanes, "lanes") | _log2_lanes(z_lanes, "z_lanes") << 4
    if offsets is not None:
        head = _IMAGE_HEADER.pack(IMAGE_PMAGIC, IMAGE_VERSION, img_size, K, patch, nib, overlap, width, height, chunk,
                                  (q & 0xFF) | len(offsets) << 8, g.T) + _offset_bytes(offsets)
    else:
        head = _IMAGE_HEADER.pack(IMAGE_QMAGIC if q else IMAGE_MAGIC, IMAGE_VERSION, img_size, K, patch, nib, overlap,
                                  width, height, chunk, q & 0xFF, g.T)
    return head + b"".join(table) + b"".join(body)


def _image_q(magic, word):
    """bytes 18-19 of a TMT / TQT header (as the u16 `word`) -> q: TMT holds zero there, TQT q as int8 then zero"""
    if magic == IMAGE_MAGIC:
        if word:
            raise ValueError(f"reserved bytes 18-19 hold {word:#06x}, must be zero")
        return 0
    q = _read_q(word & 0xFF, "TQT", "TMT")
    if word >> 8:
        raise ValueError(f"TQT stream: padding byte 19 holds {word >> 8:#04x}, must be zero")
    return q


def parse_image(blob) -> ImageBlob:
    """header fields and per-tile views of a TMT file; ValueError on anything that is not a well-formed version-1
    file (the records themselves are checked by the coder)"""
    from .tiling import MAX_TILES, grid

    mv = memoryview(blob).cast("B") if not isinstance(blob, memoryview) else blob.cast("B")
    n = len(mv)
    if n < IMAGE_HEADER_BYTES:
        raise ValueError(f"{n} bytes: shorter than the {IMAGE_HEADER_BYTES}-byte header")
    magic, version, S, K, patch, nib, O, width, height, chunk, zero, T = _IMAGE_HEADER.unpack_from(mv, 0)
    if magic not in (IMAGE_MAGIC, IMAGE_QMAGIC, IMAGE_PMAGIC):
        raise ValueError(f"not a TMT bitstream (magic {bytes(magic)!r})")
    if version != IMAGE_VERSION:
        raise ValueError(f"container version {version}, this reader knows version {IMAGE_VERSION}")
    if n % 4:
        raise ValueError(f"{n} bytes: not a whole number of 32-bit words")
    L = _check_geometry(S, K, patch)
    ll, zl = nib & 15, nib >> 4
    if ll > MAX_LANE_LOG2 or zl > MAX_LANE_LOG2:
        raise ValueError(f"lane fields 2^{ll} / 2^{zl}: at most 2^{MAX_LANE_LOG2} lanes")
    if O > S // 2:
        raise ValueError(f"overlap {O} above half the tile size {S}")
    if width == 0 or height == 0:
        raise ValueError(f"image size {width}x{height}: width and height must be >= 1")
    if chunk == 0:
        raise ValueError("chunk 0: the encoder's tile batch must be >= 1")
    hb, nlev, offsets = IMAGE_HEADER_BYTES, 1, ()
    if magic == IMAGE_PMAGIC:
        hb = IMAGE_PHEADER_BYTES
        if n < hb:
            raise ValueError(f"{n} bytes: shorter than the {hb}-byte TPT header")
        q, offsets = _read_table(zero & 0xFF, zero >> 8, mv[IMAGE_HEADER_BYTES:hb], "TPT")
        nlev = len(offsets)
    else:
        q = _image_q(magic, zero)
    if T > MAX_TILES:
        raise ValueError(f"{T} tiles: at most {MAX_TILES}")
    g = grid(height, width, S, O)
    if T != g.T:
        raise ValueError(f"{T} tiles, but {width}x{height} at tile size {S}, overlap {O} has {g.ny} x {g.nx} = {g.T}")
    body0 = hb + 8 * T
    if n < body0:
        raise ValueError(f"{n} bytes: the header and the table of {T} tiles take {body0}")
    table = np.frombuffer(mv, dtype="<u4", count=2 * T, offset=hb).reshape(T, 2)
    for t in range(T):
        if table[t, 0] < 2 or table[t, 1] < 2:
            raise ValueError(f"tile {t}: z record of {table[t, 0]} and y record of {table[t, 1]} words, each holds at "
                             f"least 2")
    W, W2 = id_words(L, K), level_words(K, nlev)
    need = body0 + 4 * (T * (W + W2) + int(table.sum(dtype=np.int64)))
    if n != need:
        raise ValueError(f"{n} bytes: the header, the table and the {T} tiles it lists take {need}")
    ids, zs, ys, lvs, at = [], [], [], [], body0
    for t in range(T):
        ids.append(np.frombuffer(mv, dtype="<u4", count=W, offset=at))
        lvs.append(np.frombuffer(mv, dtype="<u4", count=W2, offset=at + 4 * W))
        z0 = at + 4 * (W + W2)
        y0 = z0 + 4 * int(table[t, 0])
        at = y0 + 4 * int(table[t, 1])
        zs.append(mv[z0:y0])
        ys.append(mv[y0:at])
    return ImageBlob(S, K, patch, 1 << ll, 1 << zl, O, width, height, chunk, ids, zs, ys, q, nlev, offsets,
                     lvs if nlev > 1 else None)


class ImageIndex(NamedTuple):
    """read_image_index()'s result: the header fields of ImageBlob, then per tile the byte offsets of its sections in
    the file (prefix sums of the table): tile t is bytes ids_at[t] .. end_at[t], its z record starts at z_at[t] and
    its y record at y_at[t]"""
    img_size: int
    num_keep_patches: int
    patch_size: int
    lanes: int
    z_lanes: int
    overlap: int
    width: int
    height: int
    chunk: int
    ids_at: np.ndarray       # int64 [T] each
    z_at: np.ndarray
    y_at: np.ndarray
    end_at: np.ndarray
    q: int = 0               # as ImageBlob.q
    nlev: int = 1            # as ImageBlob.nlev
    offsets: tuple = ()      # as ImageBlob.offsets; a tile's level words lie between its id words and z_at[t]

    @property
    def num_tiles(self) -> int:
        return len(self.ids_at)

    @property
    def nbytes(self) -> int:
        return int(self.end_at[-1])


def _source(src):
    """(length in bytes, read(offset, size) -> bytes-like) of a bytes-like object or a seekable binary file object;
    a file is only ever read at the ranges asked for"""
    if hasattr(src, "seek") and hasattr(src, "read"):
        n = src.seek(0, 2)

        def read(at, size):
            src.seek(at)
            b = src.read(size)
            if len(b) != size:
                raise ValueError(f"read {len(b)} of the {size} bytes at offset {at}: the file changed or is not in "
                                 f"binary mode")
            return b

        return n, read
    mv = memoryview(src).cast("B") if not isinstance(src, memoryview) else src.cast("B")
    return len(mv), lambda at, size: mv[at:at + size]


def read_image_index(src) -> ImageIndex:
    """the header and the table of a TMT file without its tiles (region decode): src is a bytes-like
    object or a seekable binary file object, of which only the 24 header bytes (40 of a TPT file) and the 8 * T table
    bytes are read (the length comes from a seek to the end).  Accepts the files parse_image accepts, with its ValueErrors for
    every malformed field."""
    from .tiling import MAX_TILES, grid

    n, read = _source(src)
    if n < IMAGE_HEADER_BYTES:
        raise ValueError(f"{n} bytes: shorter than the {IMAGE_HEADER_BYTES}-byte header")
    magic, version, S, K, patch, nib, O, width, height, chunk, zero, T = _IMAGE_HEADER.unpack(
        read(0, IMAGE_HEADER_BYTES))
    if magic not in (IMAGE_MAGIC, IMAGE_QMAGIC, IMAGE_PMAGIC):
        raise ValueError(f"not a TMT bitstream (magic {bytes(magic)!r})")
    if version != IMAGE_VERSION:
        raise ValueError(f"container version {version}, this reader knows version {IMAGE_VERSION}")
    if n % 4:
        raise ValueError(f"{n} bytes: not a whole number of 32-bit words")
    L = _check_geometry(S, K, patch)
    ll, zl = nib & 15, nib >> 4
    if ll > MAX_LANE_LOG2 or zl > MAX_LANE_LOG2:
        raise ValueError(f"lane fields 2^{ll} / 2^{zl}: at most 2^{MAX_LANE_LOG2} lanes")
    if O > S // 2:
        raise ValueError(f"overlap {O} above half the tile size {S}")
    if width == 0 or height == 0:
        raise ValueError(f"image size {width}x{height}: width and height must be >= 1")
    if chunk == 0:
        raise ValueError("chunk 0: the encoder's tile batch must be >= 1")
    hb, nlev, offsets = IMAGE_HEADER_BYTES, 1, ()
    if magic == IMAGE_PMAGIC:
        hb = IMAGE_PHEADER_BYTES
        if n < hb:
            raise ValueError(f"{n} bytes: shorter than the {hb}-byte TPT header")
        q, offsets = _read_table(zero & 0xFF, zero >> 8, read(IMAGE_HEADER_BYTES, hb - IMAGE_HEADER_BYTES), "TPT")
        nlev = len(offsets)
    else:
        q = _image_q(magic, zero)
    if T > MAX_TILES:
        raise ValueError(f"{T} tiles: at most {MAX_TILES}")
    g = grid(height, width, S, O)
    if T != g.T:
        raise ValueError(f"{T} tiles, but {width}x{height} at tile size {S}, overlap {O} has {g.ny} x {g.nx} = {g.T}")
    body0 = hb + 8 * T
    if n < body0:
        raise ValueError(f"{n} bytes: the header and the table of {T} tiles take {body0}")
    table = np.frombuffer(read(hb, 8 * T), dtype="<u4").reshape(T, 2).astype(np.int64)
    for t in range(T):
        if table[t, 0] < 2 or table[t, 1] < 2:
            raise ValueError(f"tile {t}: z record of {table[t, 0]} and y record of {table[t, 1]} words, each holds at "
                             f"least 2")
    W = id_words(L, K) + level_words(K, nlev)
    end_at = body0 + 4 * np.cumsum(W + table.sum(axis=1))
    if n != end_at[-1]:
        raise ValueError(f"{n} bytes: the header, the table and the {T} tiles it lists take {end_at[-1]}")
    ids_at = np.concatenate([[body0], end_at[:-1]])
    z_at = ids_at + 4 * W
    return ImageIndex(S, K, patch, 1 << ll, 1 << zl, O, width, height, chunk, ids_at, z_at, z_at + 4 * table[:, 0],
                      end_at, q, nlev, offsets)


def read_tiles(src, index: ImageIndex, tiles):
    """(ids, z, y) of the listed tiles of the file read_image_index(src) gave the index of: per tile the uint32 [W]
    id words and the two records, as parse_image gives them; for a TPT file (index.nlev > 1) a fourth list follows,
    the tiles' uint32 [W2] level words.  Reads one byte range per tile and nothing else."""
    n, read = _source(src)
    if n != index.nbytes:
        raise ValueError(f"{n} bytes, but the index is of a file of {index.nbytes}")
    ids, zs, ys, lvs = [], [], [], []
    W2 = level_words(index.num_keep_patches, index.nlev)
    for t in tiles:
        t = int(t)
        if not 0 <= t < index.num_tiles:
            raise ValueError(f"tile {t} outside 0..{index.num_tiles - 1}")
        at, z0, y0, end = (int(a[t]) for a in (index.ids_at, index.z_at, index.y_at, index.end_at))
        body = memoryview(read(at, end - at))
        W = (z0 - at) // 4 - W2
        ids.append(np.frombuffer(body, dtype="<u4", count=W))
        lvs.append(np.frombuffer(body, dtype="<u4", count=W2, offset=4 * W))
        zs.append(body[z0 - at:y0 - at])
        ys.append(body[y0 - at:])
    return (ids, zs, ys, lvs) if index.nlev > 1 else (ids, zs, ys)


def tile_blob(parsed: ImageBlob, t: int) -> bytes:
    """the version-1 TMC blob of tile t of a parsed TMT file, the TQC blob of a tile of a TQT file or the TPC blob of
    a tile of a TPT file (no original size): what MCM.encode_bytes gives for that tile, and what parse() /
    MCM.decode_bytes read"""
    p = parsed
    if not 0 <= t < p.num_tiles:
        raise ValueError(f"tile {t} outside 0..{p.num_tiles - 1}")
    if p.nlev > 1:
        return assemble(p.img_size, p.num_keep_patches, p.patch_size, p.lanes, p.z_lanes, None, p.ids[t], p.z[t],
                        p.y[t], p.q, p.offsets, p.levels[t])
    return assemble(p.img_size, p.num_keep_patches, p.patch_size, p.lanes, p.z_lanes, None, p.ids[t], p.z[t], p.y[t],
                    p.q)


def pack_ids_host(ids_keep, L: int) -> np.ndarray:
    """ids_keep [K] or [n, K] (each id in [0, L)) -> uint32 words [W] or [n, W]: tmae_ids_pack in numpy"""
    ids = np.asarray(ids_keep, dtype=np.int64)
    one = ids.ndim == 1
    ids = np.atleast_2d(ids)
    n, K = ids.shape
    bits = id_bits(L)
    if not 1 <= K <= L or (ids < 0).any() or (ids >= L).any():
        raise ValueError(f"pack_ids_host: need 1 <= K={K} <= L={L} and every id in [0, L)")
    W = id_words(L, K)
    # the bit string, one byte per bit, LSB of id k at position k * bits
    string = np.zeros((n, 32 * W), dtype=np.uint8)
    string[:, :K * bits] = ((ids[:, :, None] >> np.arange(bits)) & 1).reshape(n, K * bits)
    words = (string.reshape(n, W, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)
    return words[0] if one else words


def unpack_ids_host(words, L: int, K: int):
    """words uint32 [W] or [n, W] -> (ids_shuffle, ids_restore int64 [L] or [n, L], status int32 scalar or [n]):
    tmae_ids_unpack in numpy.  The kept ids, then the unused ones ascending; status 0 ok, 1 id >= L, 2 duplicate id,
    3 non-zero tail bits (the lowest that applies), and the identity in both outputs wherever it is not 0."""
    w = np.asarray(words).astype(np.uint32, copy=False)
    one = w.ndim == 1
    w = np.atleast_2d(w)
    n, bits = w.shape[0], id_bits(L)
    if not 1 <= K <= L or w.shape[1] != id_words(L, K):
        raise ValueError(f"unpack_ids_host: need 1 <= K={K} <= L={L} and {id_words(L, K)} words per image")
    string = ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(n, -1).astype(np.int64)
    ids = (string[:, :K * bits].reshape(n, K, bits) << np.arange(bits)).sum(axis=2)
    shuf = np.tile(np.arange(L, dtype=np.int64), (n, 1))
    rest = shuf.copy()
    status = np.zeros(n, dtype=np.int32)
    for b in range(n):
        if (ids[b] >= L).any():
            status[b] = 1
        elif np.unique(ids[b]).size != K:
            status[b] = 2
        elif string[b, K * bits:].any():
            status[b] = 3
        else:
            unused = np.setdiff1d(np.arange(L), ids[b])  # ascending
            shuf[b] = np.concatenate([ids[b], unused])
            rest[b, shuf[b]] = np.arange(L)
    return (shuf[0], rest[0], status[0]) if one else (shuf, rest, status)


# ------------------------------------------------------------------ per-patch quantiser steps: the kernels in numpy
# csrc/qlevels.hip restated; integers and comparisons only, so the tests compare with equality.
def select_levels_host(ids_shuffle, K: int, nlev: int, scores=None, level_map=None):
    """tmae_qlevels_select in numpy: ids_shuffle int [n, L] and either scores f32 [n, L] or level_map int [n, L] ->
    (levels int32 [n, K], status int32 [n]).  Scores: s[p] = scores[b][ids_shuffle[b][p]], rank r[p] = #{p' : s[p'] >
    s[p] or (s[p'] == s[p] and p' < p)}, level = r nlev // K.  Map: the gathered entries; one outside 0..nlev-1 ->
    status 1 and all-zero levels for the image"""
    ids = np.atleast_2d(np.asarray(ids_shuffle, dtype=np.int64))
    n, L = ids.shape
    if not 1 <= K <= L <= MAX_L or not NLEV_MIN <= nlev <= NLEV_MAX or (scores is None) == (level_map is None):
        raise ValueError(f"select_levels_host: need 1 <= K={K} <= L={L} <= {MAX_L}, nlev={nlev} in {NLEV_MIN}.."
                         f"{NLEV_MAX} and exactly one of scores and level_map")
    keep = ids[:, :K]
    status = np.zeros(n, dtype=np.int32)
    if level_map is not None:
        lv = np.take_along_axis(np.asarray(level_map, dtype=np.int64).reshape(n, L), keep, axis=1)
        bad = ((lv < 0) | (lv >= nlev)).any(axis=1)
        status[bad] = 1
        lv[bad] = 0
        return lv.astype(np.int32), status
    s = np.take_along_axis(np.asarray(scores, dtype=np.float32).reshape(n, L), keep, axis=1)
    with np.errstate(invalid="ignore"):
        a, b = s[:, None, :], s[:, :, None]                      # a[.., p'] against b[.., p]
        earlier = np.arange(K)[None, None, :] < np.arange(K)[None, :, None]
        r = ((a > b) | ((a == b) & earlier)).sum(axis=2)
    return ((r * nlev) // K).astype(np.int32), status


def pack_levels_host(levels, nlev: int) -> np.ndarray:
    """levels [K] or [n, K] (each in [0, nlev)) -> uint32 words [W2] or [n, W2]: tmae_qlevels_pack in numpy"""
    lv = np.asarray(levels, dtype=np.int64)
    one = lv.ndim == 1
    lv = np.atleast_2d(lv)
    n, K = lv.shape
    if not NLEV_MIN <= nlev <= NLEV_MAX or K < 1 or (lv < 0).any() or (lv >= nlev).any():
        raise ValueError(f"pack_levels_host: need nlev={nlev} in {NLEV_MIN}..{NLEV_MAX} and every level in [0, nlev)")
    bits, W = level_bits(nlev), level_words(K, nlev)
    string = np.zeros((n, 32 * W), dtype=np.uint8)
    string[:, :K * bits] = ((lv[:, :, None] >> np.arange(bits)) & 1).reshape(n, K * bits)
    words = (string.reshape(n, W, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)
    return words[0] if one else words


def unpack_levels_host(words, nlev, K: int):
    """tmae_qlevels_unpack in numpy: words uint32 [n, ldw] (rows padded to a common width) and nlev int [n] (or one int
    for all) -> (levels int32 [n, K], status int32 [n]): 0 ok, 1 a level >= nlev, 2 non-zero tail bits (the lowest that
    applies), all-zero levels wherever it is not 0; nlev[b] == 1: no map, nothing read, all levels 0"""
    w = np.atleast_2d(np.asarray(words)).astype(np.uint32, copy=False)
    n, ldw = w.shape
    nl = np.broadcast_to(np.asarray(nlev, dtype=np.int64), (n,))
    levels = np.zeros((n, K), dtype=np.int32)
    status = np.zeros(n, dtype=np.int32)
    for b in range(n):
        v = int(nl[b])
        if v == 1:
            continue
        W = level_words(K, v) if 2 <= v <= NLEV_MAX else ldw + 1
        if W > ldw:
            status[b] = 1
            continue
        bits = level_bits(v)
        string = ((w[b, :W, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(-1).astype(np.int64)
        lv = (string[:K * bits].reshape(K, bits) << np.arange(bits)).sum(axis=1)
        if (lv >= v).any():
            status[b] = 1
        elif string[K * bits:].any():
            status[b] = 2
        else:
            levels[b] = lv
    return levels, status


def build_qmap_host(levels, q, offsets) -> np.ndarray:
    """tmae_qmap_build in numpy: qmap[b][p] = clamp(q[b] + offsets[b][levels[b][p]], Q_MIN, Q_MAX) -> int32 [n, K];
    levels int [n, K], q int [n] or None (all zero), offsets int [n, 16] (or one row for all images)"""
    lv = np.atleast_2d(np.asarray(levels, dtype=np.int64))
    n = lv.shape[0]
    off = np.broadcast_to(np.asarray(offsets, dtype=np.int64), (n, NLEV_MAX))
    base = np.zeros(n, dtype=np.int64) if q is None else np.broadcast_to(np.asarray(q, dtype=np.int64), (n,))
    return np.clip(base[:, None] + np.take_along_axis(off, lv & (NLEV_MAX - 1), axis=1), Q_MIN, Q_MAX).astype(np.int32)


def offsets_row(offsets) -> list:
    """the 16 ints of tmae_qmap_build's table row: the offsets, then zeros (an image without a map: all zero)"""
    return list(offsets) + [0] * (NLEV_MAX - len(offsets))
