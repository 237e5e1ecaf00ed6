"""Shapes shared by tests/test_gpu_trajectories.py and tests/test_trajectories_host.py (no GPU, no other test module needed): name -> (N, dims).
The first six are SHAPES of tests/test_gpu_instance_cost.py (the GPU test asserts that they still are); "ny0" has no output; "odd3" has
N nx + N ny = 105 (not a multiple of 16: the last block of 16 rows is partial and one block straddles x and y) and an inner dimension of
252 + 3 + 273 + 1 = 529 (three chunks of 256)."""

SHAPES = {
    "below16": (5, dict(nx=3, nu=1, ndelta=1, nz=1, nomega=3, ny=3, nc=4)),
    "straddle64": (13, dict(nx=5, nu=3, ndelta=1, nz=1, nomega=5, ny=1, nc=4)),
    "nx17": (4, dict(nx=17, nu=14, ndelta=1, nz=1, nomega=16, ny=4, nc=4)),
    "nw0": (9, dict(nx=7, nu=5, ndelta=1, nz=1, nomega=0, ny=2, nc=3)),
    "nx0": (6, dict(nx=0, nu=4, ndelta=1, nomega=4, ny=3, nc=4)),
    "k380": (20, dict(nx=17, nu=2, ndelta=1, nz=1, nomega=2, ny=2, nc=3)),
    "ny0": (7, dict(nx=6, nu=3, ndelta=1, nz=1, nomega=2, ny=0, nc=3)),
    "odd3": (21, dict(nx=3, nu=10, ndelta=1, nz=1, nomega=13, ny=2, nc=3)),
}
TV_SHAPE = (8, dict(nx=4, nu=3, ndelta=1, nmu=1, nomega=2, ny=2, nc=4))
