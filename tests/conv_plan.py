"""The dispatch rule of csrc/conv2d.hip's implicit-GEMM kernel, restated plainly, and the case table of tests/test_conv_forms_gpu.py.  No device,
no torch: tests/test_conv_plan_cpu.py holds this file to the source's constants and the table to the (entry, form, arm) matrix.

conv2d_mfma_kernel<MAP, TM, TN, NBUF, FG, VEC, EP> is instantiated by dispatch_conv_mfma / dispatch_conv_project from the shape alone:
  S   depth <= CV_SHORT_K                                      64 x 64 tile, two LDS buffers, a partial sum every 8 terms
  M   depth >  CV_SHORT_K, fewer than CV_LARGE_TILES tiles     64 x 64 tile, two LDS buffers, a partial sum every 32 terms
  L   depth >  CV_SHORT_K, at least CV_LARGE_TILES tiles       128 x 128 tile, one LDS buffer, two barriers, a partial sum every 32 terms
where "tiles" counts 128 x 128 tiles of the rows x cols problem.  The project entry has one 64-wide column tile and never takes L.
rows, cols and depth per slot map (FwdMap / BwdMap / TransMap):
  Fwd    Ho Wo    Cout       k k Cin
  Bwd    Hi Wi    Cin        k k Cout
  Trans  H W      s s Cout   Cin
The load arm is "vec" (16-byte loads) when the A and B base pointers are 16-byte multiples and the A leading dimension is a multiple of 4,
"scalar" otherwise; the other pointers and leading dimensions do not enter."""

CV_SHORT_K = 1024
CV_LARGE_TILES = 512

MAPS = ("Fwd", "Bwd", "Trans")
FORMS = ("S", "M", "L")
ARMS = ("vec", "scalar")


def conv_out_size(n, k, s, p, d=1):
    span = n + 2 * p - d * (k - 1) - 1
    return 0 if span < 0 else span // s + 1


def large_tiles(rows, cols):
    return -(-rows // 128) * -(-cols // 128)


def plan(map, rows, cols, depth):
    """the form dispatch_conv_mfma<MAP> launches"""
    assert map in MAPS and rows >= 1 and cols >= 1 and depth >= 1
    if depth <= CV_SHORT_K:
        return "S"
    return "L" if large_tiles(rows, cols) >= CV_LARGE_TILES else "M"


def plan_project(depth):
    """the form dispatch_conv_project launches"""
    return "S" if depth <= CV_SHORT_K else "M"


def arm(ptrs, ld):
    """ptrs = the byte addresses of the A operand (x / grad_out) and of the packed weight; ld = the A operand's leading dimension in floats"""
    return "vec" if all(p % 16 == 0 for p in ptrs) and ld % 4 == 0 else "scalar"


def extents(map, H, W, cin, cout, k=1, s=1, p=0):
    """(rows, cols, depth) of the implicit GEMM.  H, W: the input image of Fwd and Trans, and the image whose gradient Bwd computes.
    Trans takes its stride s as the kernel."""
    if map == "Fwd":
        return conv_out_size(H, k, s, p) * conv_out_size(W, k, s, p), cout, k * k * cin
    if map == "Bwd":
        return H * W, cin, k * k * cout
    if map == "Trans":
        return H * W, s * s * cout, cin
    raise ValueError(map)


# The entries (rows of the coverage matrix) and the slot map each one instantiates.  A "Fwd" case of the table runs through dr_conv2d_rows_f32
# and dr_conv2d_rows_act_f32 both, a "PROJECT" case through dr_conv2d_rows_project_f32.
ENTRIES = {"Fwd/plain": "Fwd", "Fwd/ACT": "Fwd", "Bwd": "Bwd", "Trans": "Trans", "Fwd/PROJECT": "Fwd"}


def reachable_cells():
    cells = [(e, f, a) for e in ("Fwd/plain", "Fwd/ACT", "Bwd", "Trans") for f in FORMS for a in ARMS]
    return cells + [("Fwd/PROJECT", f, a) for f in ("S", "M") for a in ARMS]


def case(id, entry, form, why, pair=None, **geom):
    return dict(id=id, entry=entry, form=form, why=why, pair=pair, geom=geom)


# The case table of tests/test_conv_forms_gpu.py: the smallest shapes that select each form and stay ragged at every tile edge.  Every case runs on
# both load arms.  pair = the case whose inputs this one shares (its first H image rows): the two sides of the tile-count threshold.
CASES = [
    case("fwd_S_k1024", "Fwd", "S", "pointwise, depth 1 024 = CV_SHORT_K exactly: the last depth of the 8-term window",
         H=3, W=5, cin=1024, cout=20, k=1, s=1, p=0),
    case("fwd_M_k1028", "Fwd", "M", "pointwise, depth 1 028: the other side of CV_SHORT_K, a 4-wide last chunk",
         H=3, W=5, cin=1028, cout=20, k=1, s=1, p=0),
    case("fwd_M", "Fwd", "M", "K = 1 044 = 32 chunks + 20 (a tail that is no multiple of 8); column tiles 64 + 4; row tiles 64 + 64 + 15",
         H=13, W=11, cin=116, cout=68, k=3, s=1, p=1),
    case("fwd_L", "Fwd", "L", "32 761 pixels = 256 row tiles x 2 column tiles = 512, the threshold; last row tile 121 rows, last column tile 4",
         H=181, W=181, cin=116, cout=132, k=3, s=1, p=1),
    case("fwd_M_510", "Fwd", "M", "255 x 2 = 510 large tiles: the other side of CV_LARGE_TILES", pair="fwd_L",
         H=180, W=181, cin=116, cout=132, k=3, s=1, p=1),
    case("bwd_M", "Bwd", "M", "stride 2: a gather with holes on the 32-term window; depth 1 044, 567 pixels, 20 columns",
         H=21, W=27, cin=20, cout=116, k=3, s=2, p=1),
    case("bwd_L", "Bwd", "L", "the data gradient on the single-buffer tile: 256 x 2 = 512 large tiles, depth 1 044",
         H=181, W=181, cin=132, cout=116, k=3, s=1, p=1),
    case("bwd_M_510", "Bwd", "M", "255 x 2 = 510 large tiles: the other side of CV_LARGE_TILES", pair="bwd_L",
         H=180, W=181, cin=132, cout=116, k=3, s=1, p=1),
    case("trans_S", "Trans", "S", "the scalar arm of the transposed convolution on the short window (no earlier test runs it)",
         H=5, W=7, cin=36, cout=20, s=2),
    case("trans_M", "Trans", "M", "depth 1 028 > 1 024 with a 4-wide last chunk; 35 pixels, 80 columns",
         H=5, W=7, cin=1028, cout=20, s=2),
    case("trans_L", "Trans", "L", "8 row tiles x 65 column tiles = 520; last row tile 3 rows, last column tile 64 columns; pixel shuffle s = 4",
         H=29, W=31, cin=1028, cout=516, s=4),
    case("project_S", "Fwd/PROJECT", "S", "Cmid 36 on the 8-term window, K = 324; the scalar arm is new",
         H=5, W=7, cin=36, cout=36, k=3, s=1, p=1),
    case("project_M", "Fwd/PROJECT", "M", "Cmid 36 on the 32-term window, K = 1 152; the scalar arm is new",
         H=5, W=7, cin=128, cout=36, k=3, s=1, p=1),
]
BY_ID = {c["id"]: c for c in CASES}


def entries_of(c):
    return ("Fwd/plain", "Fwd/ACT") if c["entry"] == "Fwd" else (c["entry"],)


def case_extents(c):
    return extents(ENTRIES[entries_of(c)[0]], **c["geom"])


def case_plan(c):
    rows, cols, depth = case_extents(c)
    return plan_project(depth) if c["entry"] == "Fwd/PROJECT" else plan(ENTRIES[entries_of(c)[0]], rows, cols, depth)


def claim(file, test, entry, arm, name=None, **geom):
    return dict(file=file, test=test, entry=entry, arm=arm, name=name, geom=geom)


# What the suite reached before the table above, one claim per cell it reached, read from the tests' shapes: (file, test function, entry, arm,
# the geometry).  name = the key of image_backbone2d3d_ref.CONV_CASES the test is parametrised by, where it is; the CPU test holds the geometry
# written here to that table and every claim to plan().  (dr_conv2d_rows_f32 also ran form M, 16-byte arm, inside
# test_image_backbone2d3d_gpu.py::test_backbone_real_widths, under that test's end-to-end bar only; it is not claimed as a primitive-level check.)
_IB, _IBB, _DPT = "test_image_backbone2d3d_gpu.py", "test_image_backbone2d3d_bwd_gpu.py", "test_dpt2d3d_gpu.py"
EXISTING = [
    claim(_IB, "test_conv_against_torch", "Fwd/plain", "vec", name="ragged", H=13, W=11, cin=20, cout=160, k=3, s=1, p=1),
    claim(_IB, "test_conv_without_bias_with_addend_and_leading_dimensions", "Fwd/plain", "scalar", name="ragged",
          H=13, W=11, cin=20, cout=160, k=3, s=1, p=1),
    claim(_IB, "test_conv_against_torch", "Fwd/plain", "vec", name="large_tile", H=240, W=280, cin=128, cout=16, k=3, s=1, p=1),
    claim(_DPT, "test_act_against_torch", "Fwd/ACT", "vec", H=33, W=35, cin=64, cout=132, k=3, s=1, p=1),
    claim(_DPT, "test_act_leading_dimensions_and_unaligned_base", "Fwd/ACT", "scalar", H=5, W=7, cin=36, cout=68, k=3, s=1, p=1),
    claim(_IBB, "test_conv_gradients_against_torch", "Bwd", "vec", name="stride2", H=21, W=27, cin=16, cout=32, k=3, s=2, p=1),
    claim(_IBB, "test_conv_gradients_with_leading_dimensions_and_unaligned_pointers", "Bwd", "scalar", name="stride2",
          H=21, W=27, cin=16, cout=32, k=3, s=2, p=1),
    claim(_IBB, "test_conv_gradients_against_torch", "Bwd", "vec", name="ragged", H=13, W=11, cin=20, cout=160, k=3, s=1, p=1),
    claim(_IBB, "test_conv_gradients_with_leading_dimensions_and_unaligned_pointers", "Bwd", "scalar", name="ragged",
          H=13, W=11, cin=20, cout=160, k=3, s=1, p=1),
    claim(_DPT, "test_transpose_against_torch", "Trans", "vec", H=10, W=13, cin=36, cout=20, s=2),
    claim(_DPT, "test_project_against_float64", "Fwd/PROJECT", "vec", H=5, W=7, cin=36, cout=36, k=3, s=1, p=1),
    claim(_DPT, "test_project_against_float64", "Fwd/PROJECT", "vec", H=5, W=7, cin=128, cout=36, k=3, s=1, p=1),
]


def claim_plan(c):
    rows, cols, depth = extents(ENTRIES[c["entry"]], **c["geom"])
    return plan_project(depth) if c["entry"] == "Fwd/PROJECT" else plan(ENTRIES[c["entry"]], rows, cols, depth)


def coverage():
    """{cell: [who reaches it]}: the table's cases (both arms each) and the earlier tests claimed above"""
    cov = {cell: [] for cell in reachable_cells()}
    for c in EXISTING:
        cov[(c["entry"], claim_plan(c), c["arm"])].append("%s::%s%s" % (c["file"], c["test"], "[%s]" % c["name"] if c["name"] else ""))
    for c in CASES:
        for e in entries_of(c):
            for a in ARMS:
                cov[(e, case_plan(c), a)].append("test_conv_forms_gpu.py[%s]" % c["id"])
    return cov
