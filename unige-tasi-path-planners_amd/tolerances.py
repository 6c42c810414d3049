"""Acceptance bounds of the parity checks on the reference's consistent set, each defined HERE and nowhere else (tests/helpers.py and
__graft_entry__.smoke() import them).

FD / SG: SURVEY.md 8(d)'s max(1e-6 * G, 2 ulp) -- and every FD / SG test asserts bit equality on top of it.

MS-DFM: 2e-6 * G.  Self-derived -- the reference holds no fixture for MS-DFM (its one recorded mission log is Field D*'s, tests/test_reference_mission.py), so this part of the parity is unpinned: the float fixed point
of DFM's update operator is not unique, and WHICH one an evaluation order lands on is already a last-bits matter between two sequential
orders of the reference's own level-1 operator as the ORACLE restates it (tools/dfm_fixed_points.py: the priority-queue order against
raster Gauss-Seidel sweeps of the same candidates differ by up to 9 ulp = 1.02e-6 on the 2048^2 maps of BASELINE config 4, seed 1003);
the restated level-0 planner does not terminate at all on one of them (seed 1000: 1e9 expansions, oracle code -75).  So 1e-6 cannot be
promised by anything that does not replay the queue's pop order; the bound is twice the measured spread.  Measured engine-vs-oracle on
those eight maps: 4-8 ulp, <= 7.5e-7.

NODE_LOCAL_ULP / DFM_LOCAL_ULP: bounds of the LOCAL criterion (tests/field_reference.py) -- how far, in units in the last place, a value
G(s) may lie from what the update operator, evaluated in float64 from its geometry, makes of the neighbours of s in the same field.
Twice the worst residual of the ORACLE's trusted values, rounded up to a whole ulp, over the maps of tests/test_field_reference.py
(seeded white-noise maps of 37 x 43, 16 x 16, 17 x 17, 1 x 40 and 3 x 2 cells, thresholds 1.0 and 0.6, every algorithm and level, four
replans each at levels 1 and 2); the factor covers seeds and sizes not tried.  Measured: Field D* / Shifted Grid 0.919 ulp, MS-DFM
1.423 ulp (1.131 on the fresh plans).  tests/test_field_reference.py::test_bounds_are_the_measurement recomputes both.  The engine's
MS-DFM fields are held to DFM_LOCAL_ULP plus the 8 ulp include/ufm.h documents at ufm_check_info (tests/test_gpu_field_reference.py).

NODE_OPERATOR_ULP / DFM_OPERATOR_ULP: the same criterion on CONSTRUCTED inputs (tests/operator_cases.py) instead of converged fields -- single
triangles at every turn of their case chain for every pair of cost bytes, 3 x 3 neighbourhoods with random, tied and unreached values.
By the same rule: twice the ORACLE's worst residual against float64 over the committed cases, rounded up to a whole ulp, and no less than
the field bound next to it.  Measured (seed 20): node planners 1.493 ulp (Shifted Grid, family T at `f = b sqrt 2`; Field D* 1.296 at
`f = b`; the neighbourhood families 1.236 at most), MS-DFM 1.830 ulp (family Q, random wide; obstacles 1.547) -> 3 and 4.  Arbitrary inputs
reach rounding patterns fixed points do not, hence one more ulp than the field bounds.  tests/test_operator_cases.py::
test_operator_bounds_are_the_measurement recomputes both; tests/test_gpu_operators.py holds the device functions of csrc/ufm_ops.h to them
(and to the oracle bit for bit).

SCORE_FP64_CHAIN: trajectory scoring (csrc/ufm_score_rect.h) against its float64 restatement (tests/score_reference.py).  A free path's
cost, cost_before and dist are held to 0.5 ulp32(ref) -- the one narrowing to fp32 -- plus pieces * Cmax * SCORE_FP64_CHAIN * 2^-53 *
max(M, 1), the fp64 arithmetic in front of it: M the largest coordinate magnitude of the path, Cmax the dearest chargeable byte.  Derived
from the header, no measurement in it.  The correctly rounded fp64 operations between the fp32 end points and one piece's share of the
sum, in score_segment(): dx = bx - ax, dy = by - ay, dx * dx, dy * dy, their sum, the square root (6: the segment's length); for each
of the two cuts that bound the piece k - ax and the division by dx (4); tn - t0 and its product with the length (2); the product with
the cell's cost and the two additions, into the segment's sum and into the path's (3): 15.  Each is off by at most 2^-53 of a quantity
that moves the piece's length by no more than the segment's length (t0, tn <= 1), and a segment between coordinates of magnitude M is
no longer than 2 sqrt(2) M < 3 M: 15 * 3 = 45.  What this form does not cover, stated rather than hidden: the two additions act on
partial sums, not on one piece, so over a path they contribute up to (pieces + segments) * 2^-53 * ref, which exceeds a piece's share
above once a path has more than ~30 max(M, 1) pieces; both terms stay eight orders of magnitude below the half ulp32 in front, and can
only show when the exact sum lies that close to the middle between two fp32 values."""
FIELD_RTOL = 1e-6
DFM_RTOL = 2e-6
NODE_LOCAL_ULP = 2
DFM_LOCAL_ULP = 3
NODE_OPERATOR_ULP = 3
DFM_OPERATOR_ULP = 4
SCORE_FP64_CHAIN = 45
