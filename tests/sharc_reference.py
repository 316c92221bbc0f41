"""Row N14 -- the radiance cache of DESIGN.md spec S20 restated in Python (float64 and exact integers) from the spec's text, for
tests/test_sharc.py: the hash grid, the key, the hash map's find / insert / erase, the quantisation, the resolve and the query's
validity rule.  Nothing here reads csrc/pt_sharc.h."""
import math

BUCKET = 16
LEVEL_BIAS = 2
RADIANCE_SCALE = 1024.0
MAX_CONTRIBUTION = 256.0
SAMPLE_BITS, FRAME_BITS = 16, 8
MAX_SAMPLES = (1 << SAMPLE_BITS) - 1
NO_SLOT = 0xFFFFFFFF


def hash32(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def grid_level(dist2):
    """clamp(floor(log2(d2) / 2) + bias, 1, 1023); d2 a float32 value (zero, denormals: the lowest level)"""
    if not (dist2 >= 2.0 ** -126):
        return 1
    if math.isinf(dist2):
        return min(max(64 + LEVEL_BIAS, 1), 1023)
    m, e = math.frexp(dist2)          # dist2 = m 2^e, m in [0.5, 1): log2 in [e - 1, e)
    return min(max((e - 1) // 2 + LEVEL_BIAS, 1), 1023)


def voxel_size(level, scene_scale):
    return math.inf if level > 127 else 2.0 ** level / (scene_scale * 2.0 ** LEVEL_BIAS)


def cell(x, voxel):
    q = x / voxel
    g = -65536 if math.isnan(q) else (q if math.isinf(q) else math.floor(q))
    g = int(min(max(g, -65536), 65535))
    return g & 0x1FFFF


def key(P, N, level, voxel):
    level = min(max(level, 1), 1023)
    octant = (1 if N[0] < 0 else 0) | (2 if N[1] < 0 else 0) | (4 if N[2] < 0 else 0)
    return cell(P[0], voxel) | (cell(P[1], voxel) << 17) | (cell(P[2], voxel) << 34) | (level << 51) | (octant << 61)


def unpack_key(k):
    sx = lambda v: v - (1 << 17) if v & (1 << 16) else v
    return dict(cell=(sx(k & 0x1FFFF), sx((k >> 17) & 0x1FFFF), sx((k >> 34) & 0x1FFFF)), level=(k >> 51) & 0x3FF, octant=k >> 61)


def bucket_base(k, capacity):
    h = hash32((k & 0xFFFFFFFF) ^ hash32(k >> 32))
    return (h & (capacity // BUCKET - 1)) * BUCKET


class Map:
    """the hash map as the spec states it: find scans the whole bucket; insert = find, then the first empty slot in order"""

    def __init__(self, capacity):
        self.capacity, self.keys = capacity, [0] * capacity

    def find(self, k):
        b = bucket_base(k, self.capacity)
        for s in range(b, b + BUCKET):
            if self.keys[s] == k:
                return s
        return NO_SLOT

    def insert(self, k):
        s = self.find(k)
        if s != NO_SLOT:
            return s
        b = bucket_base(k, self.capacity)
        for s in range(b, b + BUCKET):
            if self.keys[s] == 0:
                self.keys[s] = k
                return s
        return NO_SLOT

    def erase(self, k):
        s = self.find(k)
        if s != NO_SLOT:
            self.keys[s] = 0
        return s


def quantise(x):
    if math.isnan(x) or not x > 0:
        return 0
    return int(math.floor(min(x, MAX_CONTRIBUTION) * RADIANCE_SCALE + 0.5))


def unpack_w(w):
    return w & MAX_SAMPLES, (w >> SAMPLE_BITS) & 0xFF, w >> (SAMPLE_BITS + FRAME_BITS)


def resolve(acc, prev, accumulation_frames, max_stale_frames):
    """-> (sums as float64 triple, samples, frames, stale, clear).  acc = (x, y, z, samples of this frame), prev = a resolved voxel."""
    pn, pf, ps = unpack_w(prev[3])
    sums = [float(acc[k]) + float(prev[k]) for k in range(3)]
    n = acc[3] + pn
    frames = pf + 1
    stale = 0 if acc[3] else ps + 1
    if stale > max_stale_frames:
        return [0.0, 0.0, 0.0], 0, 0, 0, True
    if frames > accumulation_frames:
        sums = [v * accumulation_frames / frames for v in sums]
        n0, n = n, n * accumulation_frames // frames
        if n0 and not n:
            n = 1
        frames = accumulation_frames
    while n > MAX_SAMPLES or max(sums) >= 2.0 ** 32:
        sums = [v / 2 for v in sums]
        n >>= 1
    return sums, n, frames, stale, False


def valid_hit(distance, voxel, previous_roughness):
    """Raytracing.hlsl:265-274 -> (valid, footprint)"""
    r = min(previous_roughness, 0.99)
    alpha = r * r
    footprint = distance * math.sqrt(0.5 * alpha * alpha / (1.0 - alpha * alpha))
    return distance > voxel * math.sqrt(3.0) and footprint > voxel, footprint
