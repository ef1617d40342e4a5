"""The voxelizer cases shared by tests/test_voxel_cases_cpu.py, tests/test_voxelize_cpu.py and tests/test_gpu_voxelizer.py.

Every case is one STL file, written into a temporary directory from fluid_simulation_amd/shapes.py's generators plus a few
lines of numpy, and one call of loadSTLIntoObstacles: grid, scale, rotation, translation, seed.  The GPU test compares the
mask and the count of fs_load_stl with the oracle's (oracle/cpu_ref.c, cr_load_stl) cell for cell; the CPU test shows on the
oracle alone that every case reaches what it claims.

What makes a case worth having is its "sensitive" mark.  A closed mesh sampled hundreds of times per cell hides the random
stream: any ray direction gives the same parity and a cell is marked by many samples.  An OPEN mesh mapped at about one
sample per cell (scale * min(W, H, D) close to ns) turns the mask into a picture of the stream itself: whether a sample's
ray crosses the shell once depends on its own direction, and the sample alone decides its cell.  Such a case is marked
sensitive, and the CPU test holds it to a floor: its mask and the mask of seed + 1 differ in at least 20 % of the cells of
their union.

    name        the case id
    write       write(path): creates the file
    ntri        triangles the parsers must find in it (None: the file cannot be loaded, the call returns None)
    grid        (W, H, D)
    scale, rot, translate, seed
    ns          the sample count per axis the case claims (the CPU test asserts it on the oracle)
    sensitive   held to the 20 % floor
    clip        (axis, side) of the grid face the case exists for: side 0 is cell 1, side 1 is cell N
    degenerate  the mask may be empty
    clean       a well-formed STL, fit for the compiled reference
    why         the property the case exists for
"""
import os
import struct

import numpy as np

from fluid_simulation_amd import shapes as S

M31 = 2147483647                                          # the generator's modulus
SEED_EDGES = [0, 1, M31 - 1, M31, M31 + 1, 2 ** 32 - 2, 2 ** 32 - 1]
FOLD_TO_ONE = [0, M31, M31 + 1, 2 ** 32 - 2, 2 ** 32 - 1]   # seed % M31 is 0 or 1, and 0 maps to 1


# ---- meshes ------------------------------------------------------------------------------------------------------------

def bowl(radius=0.5):
    """the lower half of sphere_triangles(radius, 16, 8): 112 triangles, open at the equator"""
    t = S.sphere_triangles(radius, 16, 8)
    t = t[t[:, :, 2].mean(axis=1) < 0]
    assert t.shape == (112, 3, 3)
    return t


def slanted_triangle():
    return np.array([[[-0.42, -0.2, -0.15], [0.4, -0.1, 0.2], [0.05, 0.45, 0.0]]], dtype=np.float32)


def bowl_slant():
    return np.concatenate([bowl(), slanted_triangle()])


def single_triangle():
    """one triangle of radius 0.5, slanted against all three axes"""
    return np.array([[[-0.5, 0.0, 0.0], [0.2, -0.4, 0.2], [0.1, 0.35, -0.3]]], dtype=np.float32)


def cube(radius=0.5):
    h = radius / np.sqrt(3.0)
    return S.box_triangles(h, h, h)


def pool():
    """1020 triangles of radius 0.5: a 24 x 12 sphere from its lowest triangle upwards (528), a 16 x 16 sphere of radius 0.3
    (480) and a cube (12).  Its first n triangles are a bowl for n < 528: open towards +z, where every ray points."""
    return np.concatenate([S.sphere_triangles(0.5, 24, 12)[::-1], S.sphere_triangles(0.3, 16, 16), cube(0.25)])


def first(n):
    return lambda: pool()[:n]


def binary(mesh):
    return lambda path: S.write_binary_stl(path, mesh())


# ---- file formats ------------------------------------------------------------------------------------------------------

def _facet(t, fmt="%.9g", indent="  ", eol="\n", count=3):
    """one ASCII facet with `count` vertex lines (the triangle's own, then its first again)"""
    out = [indent + "facet normal 0 0 0", indent * 2 + "outer loop"]
    for v in [t[0], t[1], t[2], t[0]][:count]:
        out.append(indent * 3 + "vertex " + " ".join(fmt % float(c) for c in v))
    out += [indent * 2 + "endloop", indent + "endfacet"]
    return eol.join(out) + eol


def ascii_file(mesh, counts=None, **kw):
    eol = kw.get("eol", "\n")

    def write(path):
        tris = mesh()
        with open(path, "w", newline="") as f:
            f.write("solid mesh" + eol)
            for i, t in enumerate(tris):
                f.write(_facet(t, count=(counts(i) if counts else 3), **kw))
            f.write("endsolid mesh" + eol)
    return write


def solid_header_binary(path):
    """a binary file whose 80-byte header starts with "solid": read as ASCII, no triangle in it"""
    tris = bowl()
    with open(path, "wb") as f:
        f.write(b"solid but binary".ljust(80, b" "))
        f.write(struct.pack("<I", len(tris)))
        for t in tris:
            f.write(struct.pack("<12fH", 0.0, 0.0, 0.0, *t.reshape(-1), 0))


def odd_facets(i):
    return 2 if i % 5 == 1 else (4 if i % 5 == 3 else 3)


def kept_facets(n):
    return [i for i in range(n) if odd_facets(i) == 3]


# ---- the table ---------------------------------------------------------------------------------------------------------

G = (64, 48, 40)                                          # scale 1.3: 1.3 * 40 = 52 = ns of a radius-0.5 mesh


def case(name, write, ntri, why, grid=G, scale=1.3, rot=(0.0, 0.0, 0.0), translate=(0.0, 0.0, 0.0), seed=1, ns=52,
         sensitive=False, clip=None, degenerate=False, clean=True):
    return dict(name=name, write=write, ntri=ntri, why=why, grid=grid, scale=scale, rot=rot, translate=translate, seed=seed,
                ns=ns, sensitive=sensitive, clip=clip, degenerate=degenerate, clean=clean)


def _cases():
    c = []
    # the stream decides
    c.append(case("bowl", binary(bowl), 112, "open shell at one sample per cell", sensitive=True))
    c.append(case("bowl_slant", binary(bowl_slant), 113, "a triangle crossing the shell: parities of 0, 1 and 2", sensitive=True))
    c.append(case("one_triangle", binary(single_triangle), 1, "ntri = 1: the shadow of one triangle", sensitive=True))
    c.append(case("bowl_x1000", binary(lambda: bowl(500.0)), 112,
                  "unclamped resolution (ns near 200), coordinates whose ulp is coarser than the jitter's 1e-6 steps",
                  grid=(48, 40, 44), scale=2.5, rot=(25.0, 40.0, 70.0), translate=(3.0, -2.0, 1.0), seed=7, ns=200, sensitive=True))
    # seed edges
    for s in SEED_EDGES:
        if s != 1:
            c.append(case("bowl_seed_%d" % s, binary(bowl), 112, "seed folding: seed %% (2^31 - 1), 0 -> 1", seed=s))
    # triangle-count edges around the LDS tile of 256
    for n in (12, 255, 256, 257, 512, 513, 1020):
        mesh = cube if n == 12 else first(n)
        c.append(case("tris_%d" % n, binary(mesh), n, "triangle tiles: %d = %d full + %d" % (n, n // 256, n % 256),
                      seed=3, sensitive=n in (255, 256, 257)))
    # sample-count edges
    c.append(case("ns_0", binary(lambda: S.sphere_triangles(0.005, 8, 4)), 48, "ns = 0: no sample, 0 and not None", ns=0,
                  degenerate=True))
    c.append(case("ns_1", binary(lambda: S.sphere_triangles(0.012, 8, 4)), 48, "ns = 1: one sample, at the corner", ns=1,
                  degenerate=True))
    c.append(case("ns_3", binary(lambda: S.sphere_triangles(0.03, 8, 4)), 48, "ns = 3: fewer kept samples than one block",
                  ns=3))
    c.append(case("sphere_r1", binary(lambda: S.sphere_triangles(1.0, 8, 4)), 48, "resolution clamped to 0.02: ns = 105",
                  grid=(32, 24, 20), scale=0.8, ns=105))
    c.append(case("sphere_r2", binary(lambda: S.sphere_triangles(2.0, 8, 4)), 48, "resolution span / 200, unclamped",
                  grid=(32, 24, 20), scale=0.8, ns=200))
    # mapping: one face of the grid each, a closed cube so that every sample inside has odd parity
    CG = (24, 20, 16)
    for axis, name in enumerate("xyz"):
        for side in (0, 1):
            tr = [0.0, 0.0, 0.0]
            tr[axis] = (CG[axis] / 2.0 - 1.5) * (1 if side else -1)
            c.append(case("clip_%s%s" % (name, "+" if side else "-"), binary(cube), 12,
                          "samples beyond the face %s = %s are dropped, those on it kept" % (name, "N" if side else "1"),
                          grid=CG, scale=1.5, translate=tuple(tr), clip=(axis, side), seed=5))
    c.append(case("outside", binary(cube), 12, "the whole mesh maps outside the grid: 0 added, mask untouched", grid=CG,
                  scale=0.5, translate=(100.0, 0.0, 0.0), degenerate=True))
    for g in ((40, 48, 64), (48, 40, 64), (64, 48, 40)):
        c.append(case("min_%s" % "WHD"[g.index(40)], binary(bowl), 112, "gscale takes the smallest dimension", grid=g,
                      seed=11, sensitive=True))
    for rot in ((30.0, 0.0, 0.0), (0.0, 30.0, 0.0), (0.0, 0.0, 30.0), (25.0, 40.0, 70.0)):
        c.append(case("rot_%d_%d_%d" % rot, binary(bowl), 112, "Euler rotation, host cosf / sinf", rot=rot, seed=13,
                      sensitive=True))
    # formats
    c.append(case("ascii_crlf", ascii_file(bowl, eol="\r\n"), 112, "ASCII with CRLF line ends", sensitive=True))
    c.append(case("ascii_tabs", ascii_file(bowl, indent="\t"), 112, "ASCII with leading tabs", sensitive=True))
    c.append(case("ascii_exponent", ascii_file(bowl, fmt="%.8e"), 112, "vertex lines in exponent notation", sensitive=True))
    c.append(case("ascii_2_and_4_vertices", ascii_file(bowl, counts=odd_facets), len(kept_facets(112)),
                  "a facet with two vertices is dropped; so is one with four, whose counter wraps to 0", clean=False))
    c.append(case("solid_header_binary", solid_header_binary, None, "a binary file that starts with 'solid' is ASCII: None",
                  ns=None, degenerate=True, clean=False))
    return c


CASES = _cases()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
SENSITIVE = [c for c in CASES if c["sensitive"]]
CLIP = [c for c in CASES if c["clip"]]


def ids(cases):
    return [c["name"] for c in cases]


def kwargs(c, seed=None):
    """the oracle's load_stl arguments"""
    return dict(scale=c["scale"], rot=c["rot"], translate=c["translate"], seed=c["seed"] if seed is None else seed)


# ---- malformed files (parser only) ---------------------------------------------------------------------------------------

def _records(tris):
    return b"".join(struct.pack("<12fH", 0.0, 0.0, 1.0, *np.asarray(t, dtype=np.float32).reshape(-1), 0) for t in tris)


def bad_files():
    """name -> (bytes, triangles the parsers must return)"""
    t = bowl()[:5]
    head = b"not a solid".ljust(80, b"\0")
    return {
        "empty": (b"", 0),
        "83_bytes": (head + b"\x05\0\0", 0),
        "84_bytes_count_0": (head + struct.pack("<I", 0), 0),
        "truncated_in_record_3": (head + struct.pack("<I", 5) + _records(t)[:2 * 50 + 31], 2),
        "count_ffffffff_3_records": (head + struct.pack("<I", 0xFFFFFFFF) + _records(t[:3]), 3),
        "count_2_of_5_records": (head + struct.pack("<I", 2) + _records(t), 2),
        # 1800 bytes of text are a binary file to this parser, as to the reference: a count of four characters, 34 whole
        # records.  Digits, points and spaces make floats below 2^-12: a mesh too small for one sample, and finite.
        "text_not_stl": ((" 3.25 17 42 0.001\n" * 100).encode(), (1800 - 84) // 50),
    }


def python_parse(data):
    """A plain parser written from the rules in csrc/voxelize_math.h -> float32 (n, 9)."""
    ws = b" \t\n\r"
    first_line = data.split(b"\n", 1)[0].strip(ws)
    tris = []
    if not first_line.startswith(b"solid"):
        if len(data) < 84:
            return np.zeros((0, 9), dtype=np.float32)
        n = struct.unpack_from("<I", data, 80)[0]
        n = min(n, (len(data) - 84) // 50)
        for i in range(n):
            tris.append(struct.unpack_from("<9f", data, 84 + 50 * i + 12))
    else:
        cur, vi = [None, None, None], 0
        for line in data.split(b"\n"):
            line = line.strip(ws)
            if line == b"outer loop":
                vi = 0
            elif line == b"endfacet":
                if vi == 3:
                    tris.append(tuple(cur[0] + cur[1] + cur[2]))
            elif line.startswith(b"vertex"):
                tok = line[6:].split()
                try:
                    v = tuple(float(np.float32(x.decode())) for x in tok[:3])
                except (ValueError, UnicodeDecodeError):
                    continue
                if len(v) < 3:
                    continue
                if vi < 3:
                    cur[vi] = v
                vi = (vi + 1) % 4
    return np.array(tris, dtype=np.float32).reshape(-1, 9)


# ---- shared by the tests -------------------------------------------------------------------------------------------------

def write_all(directory):
    """every case's file -> {name: path}"""
    out = {}
    for c in CASES:
        out[c["name"]] = os.path.join(str(directory), c["name"] + ".stl")
        c["write"](out[c["name"]])
    return out


def oracle_load(O, c, path, seed=None, trace=0):
    """The oracle's answer to a case -> dict(added (None: not loaded), ns, kept, mask (bool, padded), records)."""
    W, H, D = c["grid"]
    o = O.Oracle(W, H, D)
    added, ns, kept, rec = o.load_stl_traced(path, trace, **kwargs(c, seed))
    mask = o.get(O.OBS) > 0.5
    o.close()
    return dict(added=None if added < 0 else int(added), ns=ns, kept=kept, mask=mask, records=rec)


def differing_share(a, b):
    """cells that differ between two masks, as a share of the cells of their union"""
    union = int((a | b).sum())
    return (int((a ^ b).sum()) / union) if union else 0.0
