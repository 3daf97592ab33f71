"""Writer of CRFsuite 0.12 ``lCRF`` model files: the bytes a fitted ``sklearn_crfsuite.CRF`` keeps in its
``modelfile`` resource and that ``ClusterCRF.trained`` hands to the native reader (``csrc/crf_model.cpp``).

Layout, as the reader and ``oracle/lcrf.py`` parse it ([EXT] CRFsuite ``crf1d_model.c`` / ``cqdb.c``):

* a 48-byte header: ``lCRF``, total size, ``FOMC``, version 100, ``num_features`` (0: CRFsuite leaves it unset,
  the ``FEAT`` chunk carries the count), number of labels and attributes, and the offsets of the five chunks;
* ``FEAT``: 20-byte records ``(type, src, dst, weight)``, state features (type 0, ``src`` = attribute) first;
* two ``CQDB`` string <-> id databases (labels, then attributes): 24-byte header, 256 hash-table references,
  the ``(id, size, key + NUL)`` records in id order, one open-addressed table per non-empty slot (lookup3
  ``hashlittle(key + NUL, 0)``, slot = hash % 256, first bucket = (hash >> 8) % size, size = 2 x entries) and
  the id -> record back links;
* ``LFRF`` (for L + 2 labels, the last two empty) and ``AFRF``: per label the transition features leaving it, per
  attribute its state features.

`model_bytes` applies CRFsuite's save-time convention (``crf1de_save_model``): features of weight 0 are dropped,
attributes left without a feature are dropped, and what remains is renumbered in order.
"""
import struct
from typing import List, Sequence, Tuple

import numpy as np

_M32 = 0xFFFFFFFF
_CQDB_BYTEORDER = 0x62445371
_CQDB_TABLES = 256


def _rot(x: int, k: int) -> int:
    return ((x << k) | (x >> (32 - k))) & _M32


def hashlittle(key: bytes, initval: int = 0) -> int:
    """Bob Jenkins' lookup3 ``hashlittle`` (public domain), the hash CQDB keys its tables with."""
    n = len(key)
    a = b = c = (0xDEADBEEF + n + initval) & _M32
    i = 0
    while n - i > 12:
        a = (a + int.from_bytes(key[i:i + 4], "little")) & _M32
        b = (b + int.from_bytes(key[i + 4:i + 8], "little")) & _M32
        c = (c + int.from_bytes(key[i + 8:i + 12], "little")) & _M32
        a = (a - c) & _M32; a ^= _rot(c, 4); c = (c + b) & _M32  # noqa: E702
        b = (b - a) & _M32; b ^= _rot(a, 6); a = (a + c) & _M32  # noqa: E702
        c = (c - b) & _M32; c ^= _rot(b, 8); b = (b + a) & _M32  # noqa: E702
        a = (a - c) & _M32; a ^= _rot(c, 16); c = (c + b) & _M32  # noqa: E702
        b = (b - a) & _M32; b ^= _rot(a, 19); a = (a + c) & _M32  # noqa: E702
        c = (c - b) & _M32; c ^= _rot(b, 4); b = (b + a) & _M32  # noqa: E702
        i += 12
    if n - i == 0:
        return c
    tail = key[i:] + b"\0" * (12 - (n - i))
    a = (a + int.from_bytes(tail[0:4], "little")) & _M32
    b = (b + int.from_bytes(tail[4:8], "little")) & _M32
    c = (c + int.from_bytes(tail[8:12], "little")) & _M32
    c ^= b; c = (c - _rot(b, 14)) & _M32  # noqa: E702
    a ^= c; a = (a - _rot(c, 11)) & _M32  # noqa: E702
    b ^= a; b = (b - _rot(a, 25)) & _M32  # noqa: E702
    c ^= b; c = (c - _rot(b, 16)) & _M32  # noqa: E702
    a ^= c; a = (a - _rot(c, 4)) & _M32  # noqa: E702
    b ^= a; b = (b - _rot(a, 14)) & _M32  # noqa: E702
    c ^= b; c = (c - _rot(b, 24)) & _M32  # noqa: E702
    return c


def cqdb_bytes(names: Sequence[str]) -> bytes:
    """A CQDB chunk mapping ``names[i]`` <-> ``i``."""
    head = 24 + 8 * _CQDB_TABLES
    records = bytearray()
    tables: List[List[Tuple[int, int]]] = [[] for _ in range(_CQDB_TABLES)]
    back = []
    for i, name in enumerate(names):
        key = name.encode("utf-8") + b"\0"
        off = head + len(records)
        back.append(off)
        records += struct.pack("<II", i, len(key)) + key
        h = hashlittle(key)
        tables[h % _CQDB_TABLES].append((h, off))
    out = bytearray(records)
    refs = []
    for entries in tables:
        if not entries:
            refs.append((0, 0))
            continue
        n = 2 * len(entries)
        buckets = [(0, 0)] * n
        for h, off in entries:
            k = (h >> 8) % n
            while buckets[k][1] != 0:
                k = (k + 1) % n
            buckets[k] = (h, off)
        refs.append((head + len(out), n))
        for h, off in buckets:
            out += struct.pack("<II", h, off)
    bwd_offset = head + len(out)
    out += struct.pack(f"<{len(back)}I", *back)
    size = head + len(out)
    header = struct.pack("<4sIIIII", b"CQDB", size, 0, _CQDB_BYTEORDER, len(back), bwd_offset)
    header += b"".join(struct.pack("<II", o, n) for o, n in refs)
    return header + bytes(out)


def _refs_chunk(magic: bytes, base: int, lists: Sequence[Sequence[int]], n_slots: int) -> bytes:
    head = 12 + 4 * n_slots
    body = bytearray()
    offsets = [0] * n_slots
    for i, fids in enumerate(lists):
        offsets[i] = base + head + len(body)
        body += struct.pack(f"<I{len(fids)}I", len(fids), *fids)
    return struct.pack(f"<4sII{n_slots}I", magic, head + len(body), n_slots, *offsets) + bytes(body)


def lcrf_bytes(labels: Sequence[str], attrs: Sequence[str], ftype: np.ndarray, src: np.ndarray, dst: np.ndarray,
               weight: np.ndarray) -> bytes:
    """The model file for features already in CRFsuite's saved order (every state feature, by (attribute, label),
    then every transition, by (source, destination)); the features are written as given, zero weights included."""
    ftype, src, dst = (np.asarray(x, dtype=np.uint32) for x in (ftype, src, dst))
    weight = np.asarray(weight, dtype=np.float64)
    K, L, A = len(weight), len(labels), len(attrs)
    rec = np.zeros(K, dtype=np.dtype([("type", "<u4"), ("src", "<u4"), ("dst", "<u4"), ("w", "<f8")]))
    rec["type"], rec["src"], rec["dst"], rec["w"] = ftype, src, dst, weight
    feat = struct.pack("<4sII", b"FEAT", 12 + 20 * K, K) + rec.tobytes()
    lab = cqdb_bytes(labels)
    att = cqdb_bytes(attrs)
    off_feat = 48
    off_lab = off_feat + len(feat)
    off_att = off_lab + len(lab)
    off_lref = off_att + len(att)
    by_label: List[List[int]] = [[] for _ in range(L)]
    by_attr: List[List[int]] = [[] for _ in range(A)]
    for k, (t, s) in enumerate(zip(ftype.tolist(), src.tolist())):
        (by_attr if t == 0 else by_label)[s].append(k)
    lref = _refs_chunk(b"LFRF", off_lref, by_label, L + 2)
    off_aref = off_lref + len(lref)
    aref = _refs_chunk(b"AFRF", off_aref, by_attr, A)
    size = off_aref + len(aref)
    header = struct.pack("<4sI4sIIIIIIIII", b"lCRF", size, b"FOMC", 100, 0, L, A, off_feat, off_lab, off_att, off_lref,
                         off_aref)
    return header + feat + lab + att + lref + aref


def model_bytes(labels: Sequence[str], attrs: Sequence[str], state_attr: np.ndarray, state_label: np.ndarray,
                trans_src: np.ndarray, trans_dst: np.ndarray, weight: np.ndarray) -> bytes:
    """Save a trained model the way CRFsuite does.  Features are the state features ``(state_attr[k], state_label[k])``
    followed by the transitions ``(trans_src[k], trans_dst[k])``; ``weight`` holds their weights in that order.  Zero
    weights are dropped, then the attributes left without a state feature, and the remaining attributes keep their
    relative order under new ids."""
    state_attr, state_label = np.asarray(state_attr, dtype=np.int64), np.asarray(state_label, dtype=np.int64)
    trans_src, trans_dst = np.asarray(trans_src, dtype=np.int64), np.asarray(trans_dst, dtype=np.int64)
    weight = np.asarray(weight, dtype=np.float64)
    S = len(state_attr)
    if len(weight) != S + len(trans_src):
        raise ValueError("one weight per state and transition feature expected")
    ws, wt = weight[:S], weight[S:]
    keep_s, keep_t = ws != 0, wt != 0
    sa, sl, ws = state_attr[keep_s], state_label[keep_s], ws[keep_s]
    order = np.lexsort((sl, sa))
    sa, sl, ws = sa[order], sl[order], ws[order]
    ts, td, wt = trans_src[keep_t], trans_dst[keep_t], wt[keep_t]
    order = np.lexsort((td, ts))
    ts, td, wt = ts[order], td[order], wt[order]
    used = np.unique(sa)
    amap = np.full(len(attrs), -1, dtype=np.int64)
    amap[used] = np.arange(len(used))
    kept_attrs = [attrs[a] for a in used.tolist()]
    ftype = np.concatenate([np.zeros(len(sa), dtype=np.uint32), np.ones(len(ts), dtype=np.uint32)])
    return lcrf_bytes(labels, kept_attrs, ftype, np.concatenate([amap[sa], ts]), np.concatenate([sl, td]),
                      np.concatenate([ws, wt]))
