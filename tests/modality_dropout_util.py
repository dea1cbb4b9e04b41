"""CPU restatement of the per-step modality dropout (mca_pack_masks_drop, include/mca_hip.h): the numpy uint64 hash, the float32
compare, keep_one, and the padding / row masks / presence bits / drop bits expected for a list of masks.  Shared by
test_modality_dropout_cpu.py and test_modality_dropout_gpu.py; nothing here touches the package or a GPU."""
import numpy as np

M64 = (1 << 64) - 1


def fmix64(k):
    """murmur3's 64-bit finaliser on a numpy uint64 array (wrap-around multiplication)"""
    k = np.asarray(k, dtype=np.uint64).copy()
    with np.errstate(over="ignore"):
        k ^= k >> np.uint64(33)
        k *= np.uint64(0xFF51AFD7ED558CCD)
        k ^= k >> np.uint64(33)
        k *= np.uint64(0xC4CEB9FE1A85EC53)
        k ^= k >> np.uint64(33)
    return k


def uniform24(seed, step, samples, n_mod):
    """u(g, i, t) for g in samples (global sample numbers), i < n_mod -> (len(samples), n_mod) float32 in [0, 1)"""
    g = np.asarray(samples, dtype=np.int64).astype(np.uint64)[:, None]
    i = np.arange(n_mod, dtype=np.uint64)[None, :]
    h = fmix64((g << np.uint64(32)) | i)
    h = fmix64(np.uint64(int(step) & M64) ^ h)
    h = fmix64(np.uint64(int(seed) & M64) ^ h)
    return (h >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)


def draw(raw, p, seed, step, sample0=0, keep_one=True):
    """raw: (b, M) bool, modality i has a valid token in sample s before any drop; p: M rates.
    -> (dropped (b, M) bool, rescued (b,) int: the rescued modality or -1, u (b, M) float32)"""
    raw = np.asarray(raw, dtype=bool)
    b, M = raw.shape
    u = uniform24(seed, step, sample0 + np.arange(b), M)
    want = u < np.asarray(p, dtype=np.float32)[None, :]          # float32 against float32
    rescued = np.full(b, -1, dtype=np.int64)
    if keep_one:
        for s in range(b):
            if raw[s].any() and want[s][raw[s]].all():
                best = int(np.argmax(np.where(raw[s], u[s], np.float32(-1.0))))          # argmax: the first (lowest i) of equal maxima
                rescued[s] = best
                want[s, best] = False
    return want, rescued, u


def expected(masks, offsets, n_tokens, n_fusion, p, seed, step, sample0=0, keep_one=True):
    """masks: list of (b, n_i) arrays, non-zero = padded.  -> dict(padding (b, n_tokens) uint8 with 255 where the kernel writes
    nothing, rowmasks [(b * n_i,) uint8], present (b,) int32, dropped (b,) int32, matrix (b, M) bool, rescued, raw (b, M) bool, u (b, M) float32)"""
    pads = [np.asarray(m) != 0 for m in masks]
    b, M = pads[0].shape[0], len(pads)
    raw = np.stack([~pd.all(axis=1) for pd in pads], 1)
    dropped, rescued, u = draw(raw, p, seed, step, sample0, keep_one)
    padding = np.full((b, n_tokens), 255, dtype=np.uint8)
    rowmasks = []
    for i, (pd, off) in enumerate(zip(pads, offsets)):
        out = pd | dropped[:, i:i + 1]
        padding[:, off:off + pd.shape[1]] = out
        rowmasks.append(out.reshape(-1).astype(np.uint8))
    if n_fusion:
        padding[:, n_tokens - n_fusion:] = 0
    bits = lambda m: (m.astype(np.int64) << np.arange(M)[None, :]).sum(1).astype(np.int32)
    return dict(padding=padding, rowmasks=rowmasks, present=bits(raw & ~dropped), dropped=bits(dropped), matrix=dropped, rescued=rescued, raw=raw, u=u)
