"""Numpy restatement of the two-tier resident split of json3d (resident.tier_layout, csrc/json3d_cache.hip): where every frame of a
split lies, and the plan kernel's eight tables from the draw table and the split's host tables.  Copies only, so the kernel must
agree bit for bit.  test_hip_json3d_cache.py pins this restatement to the frames' pixels; test_json3d_cache_host.py pins its `img_f`
to what `json3d.pack_labels` uploads."""
import numpy as np

OUTPUTS = (("src", np.int64, ()), ("src2", np.int64, ()), ("hw", np.int32, (2,)), ("flip", np.int32, ()), ("trans_inv", np.float64, (6,)),
           ("img_i", np.int32, (7,)), ("img_f", np.float64, (19,)), ("mixed", np.uint8, ()))
DRAW_W = 18


def pad16(n):
    return (int(n) + 15) // 16 * 16


def tiers(hw, max_bytes):
    """(h, w) per frame in dataset order, the device budget -> (n_dev, device offsets, host offsets), -1 in the other tier.  Written
    as the sequential walk the layout is defined by: a frame goes to the device while no frame before it went to the host and its
    padded end still fits."""
    dev, host, used, spilled, at = [], [], 0, False, 0
    for h, w in hw:
        n = pad16(int(h) * int(w) * 3)
        if not spilled and used + n <= max_bytes:
            dev.append(used)
            host.append(-1)
            used += n
        else:
            spilled = True
            dev.append(-1)
            host.append(at)
            at += n
    return sum(o >= 0 for o in dev), np.array(dev, np.int64), np.array(host, np.int64), used, at


def staging(positions, partners, n_dev, hw):
    """the staging buffer of a batch: its distinct host-tier frames in the order rows name them (primary, then partner), each once
    -> ({position: offset}, bytes)"""
    at, n = {}, 0
    for pos, par in zip(positions, partners):
        for p in (int(pos), int(par)):
            if p >= n_dev and p not in at:
                at[p] = n
                n += pad16(int(hw[p][0]) * int(hw[p][1]) * 3)
    return at, n


def draw_rows(positions, partners, flips, scales, trans, trans_inv, staged):
    """the (B, 18) float64 draw table: [position, partner or -1, flip, scale, trans (6), trans_inv (6), staging offset of the primary and
    of the partner or -1]"""
    B = len(positions)
    d = np.zeros((B, DRAW_W), np.float64)
    d[:, 0], d[:, 1], d[:, 2], d[:, 3] = positions, partners, [int(bool(f)) for f in flips], scales
    d[:, 4:10] = np.asarray(trans, np.float64).reshape(B, 6)
    d[:, 10:16] = np.asarray(trans_inv, np.float64).reshape(B, 6)
    d[:, 16] = [staged.get(int(p), -1) for p in positions]
    d[:, 17] = [staged.get(int(p), -1) for p in partners]
    return d


def plan(base, stage, img_off, frame_hw, rec_span, P2, draws):
    """base: the arena's address (0 without one); stage: the staging buffer's (0 without one); img_off (N) int64 with -1 in the host
    tier, frame_hw (N, 2) int32 (H, W), rec_span (N, 2) int32 (first row, objects), P2 (N, 2, 12) float64 (as read, mirrored), draws
    (B, 18) float64 -> {name: array} of the kernel's eight outputs"""
    B = len(draws)
    o = {k: np.zeros((B,) + s, dt) for k, dt, s in OUTPUTS}

    def address(p, staged_at):
        if staged_at >= 0:
            return stage + int(staged_at)
        assert img_off[p] >= 0, "a host-tier frame without a staging offset"
        return base + int(img_off[p])

    for b, d in enumerate(draws):
        pos, par, fl = int(d[0]), int(d[1]), int(d[2] != 0)
        H, W = (int(v) for v in frame_hw[pos])
        o["src"][b] = address(pos, d[16])
        o["src2"][b] = address(par, d[17]) if par >= 0 else 0
        o["hw"][b] = (H, W)
        o["flip"][b] = fl
        o["trans_inv"][b] = d[10:16]
        row0, n0 = (int(v) for v in rec_span[pos])
        row1, n1 = (int(v) for v in rec_span[par]) if par >= 0 else (row0 + n0, 0)  # no partner: an empty span behind the primary's
        o["img_i"][b] = (row0, n0, row1, n1, fl, W, H)
        o["img_f"][b, :12] = P2[pos, fl]
        o["img_f"][b, 12:18] = d[4:10]
        o["img_f"][b, 18] = d[3]
        o["mixed"][b] = par >= 0
    return o
