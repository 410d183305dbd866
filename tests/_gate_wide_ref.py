"""What the tests of the router for more than 256 experts (mxmoe_moe_gate_wide, include/mxmoe_moe.h) share: the
softmax tolerance for rows of up to 513 columns and the by-construction cases. The references themselves are
tests/_gate_ref.py and tests/_gate_modes_ref.py, unchanged.
"""
from __future__ import annotations

# |w - ref| <= WIDE_SOFTMAX_RTOL * ref + 2^-126: the derivation written above _gate_ref.SOFTMAX_RTOL with 513
# summands in place of 256. A sum of up to 513 non-negative f32 terms in any order: 513 * 2^-24 ~ 3.06e-5; the
# rounded argument 5e-6; exp2 and rcp 2.4e-7; doubled for numerator over denominator: 7.2e-5, rounded up.
WIDE_SOFTMAX_RTOL = 8e-5

# (T, E, topk, n_group, topk_group, seed) of _gate_modes_ref.onehot_rows: the reference alone drops 14.1 %, 7.8 % and
# 12.5 % of the rows (margins below the scores' error bound); at most ONEHOT_MAX_DROPPED (20 %) is asserted on the CPU
WIDE_ONEHOT_CASES = [(64, 384, 8, 1, 1, 1), (64, 512, 6, 1, 1, 4), (64, 512, 8, 1, 1, 4)]
