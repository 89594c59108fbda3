"""CKKS parameter presets of the hot path (gwas/gwas.go:164-177 selects them by name; crypto.go:282-284 slots).

PN14QP438 is the preset of the reference's shipped configuration (config/configGlobal.toml:8).  The real integration takes
the moduli at run time from cryptoParams.Params.Qi()/Pi() (matmult.go:328 does the same); the values below are the
PN14QP438-shaped chain used by bench.py and the tests: q0 is the 46-bit prime the preset starts with, the others are
NTT-friendly primes (== 1 mod 2^15) of the preset's sizes."""

LOGN = 14
N = 1 << LOGN
SLOTS = N // 2
D = 91                      # ceil(sqrt(slots)), matmult.go:1047
MAX_LEVEL = 5               # maxLevel at every call site (matmult.go:42,91; pca.go:112-113; assoc.go:395,424)
DEFAULT_SCALE = 2.0 ** 34

Q_PN14 = [0x200000440001, 0x7fff80001, 0x800280001, 0x7ffd80001, 0x7ffc80001,
          0x7ff9c0001, 0x800008001, 0x7fffb0001, 0x8000f8001, 0x800250001]
P_PN14 = [0x80000050001, 0x7fffffd8001]


def rotations_for_matmul(slots=SLOTS, d=D):
    """left-rotation amounts the streamed products need keys for: baby steps 1..d-1 and giant steps d*g
    (crypto.go:252-263 generates exactly these; matmult.go:1375,1476 use them)"""
    return list(range(1, d)) + [g * d for g in range(1, d) if g * d < slots]


def generate_rot_keys(slots=SLOTS, small_dim=20, baby_flag=True):
    """crypto.GenerateRotKeys (crypto.go:232-275) as (value, right?) pairs: both sides of every power of two below the slot count, the baby and giant steps,
    right shifts below small_dim"""
    import math
    out, rot = [], 1
    l = 1
    while l < slots:
        l *= 2
    for _ in range(int(math.ceil(math.log2(l)))):
        out += [(rot, False), (rot, True)]
        rot *= 2
    if baby_flag:
        rootl = int(math.ceil(math.sqrt(slots)))
        for i in range(1, rootl):
            out += [(i, False), (i * rootl, False)]
    out += [(i, True) for i in range(1, small_dim)]
    return out


def galois_elements_for_rot_keys(rot_types=None, n=N):
    """the key set of mpc.CollectiveInit (mhe.go:70-73, 384-411): the Galois elements 5^shift of the distinct left shifts, the conjugate 2N - 1, sorted"""
    slots = n // 2
    shifts = {slots - v if right else v for v, right in (generate_rot_keys(slots) if rot_types is None else rot_types)}
    return sorted([pow(5, s, 2 * n) for s in shifts] + [2 * n - 1])
