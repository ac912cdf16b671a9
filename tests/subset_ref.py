"""numpy restatement of the gallery subsets (include/fir_amd.h, "device-side subsets of a gallery"): the row list a mask selects and
the map that takes the keys of a search over the compacted rows back to the rows they came from. Integer work only, no tolerance.
tests/test_subset_formulation.py pins both to masked_ref (pack_bits / unpack_bits / map_back)."""
import numpy as np

KEY_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
LOW = np.uint64(0xFFFFFFFF)
HIGH = np.uint64(0xFFFFFFFF00000000)


def rows_of_mask(words, n):
    """int32[count]: the LOCAL rows below n whose bit is set, ascending -- word by word, bit by bit; whatever lies at or past n is ignored."""
    words = np.asarray(words, np.uint64).reshape(-1)
    out = []
    for w in range((int(n) + 63) // 64):
        word = int(words[w])
        for b in range(64):
            r = 64 * w + b
            if r < n and (word >> b) & 1:
                out.append(r)
    return np.array(out, np.int32)


def rows_of_mask_capped(words, n, cap):
    """(count, rows[min(count, cap)]): fir_gallery_rows_of_mask's outputs -- the count is never capped."""
    rows = rows_of_mask(words, n)
    return rows.shape[0], rows[:max(int(cap), 0)]


def map_rows(keys, row_map, row_add=0, sub_offset=0):
    """fir_keys_map_rows / fir_keys_to_origin_dev: every key's low word r + sub_offset becomes uint32(row_map[r] + row_add), the
    distance bits stay, FIR_KEY_NONE stays. Returns (keys, bad): bad = a low word outside [sub_offset, sub_offset + len(row_map)) was
    met -- the host call then fails and writes nothing; the device call writes FIR_KEY_NONE there, which is what `keys` holds."""
    keys = np.asarray(keys, np.uint64)
    row_map = np.asarray(row_map, np.int64).reshape(-1)
    none = keys == KEY_NONE
    r = (keys & LOW).astype(np.int64) - int(sub_offset)
    outside = ~none & ((r < 0) | (r >= row_map.shape[0]))
    safe = np.where(none | outside, 0, r)
    target = row_map[safe] if row_map.shape[0] else np.zeros(keys.shape, np.int64)
    low = ((target + int(row_add)) % (1 << 32)).astype(np.uint64)
    mapped = np.where(none | outside, KEY_NONE, (keys & HIGH) | low)
    return mapped, bool(outside.any())
