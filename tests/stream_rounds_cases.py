"""The (plan, rows) pairs of tests/test_gpu_stream_rounds.py, kept apart from it so that the
CPU test of the planner (tests/test_tile_plan.py, `tile_plan_check rounds`) can show without a
GPU that each pair still makes pass B of the tiled engine walk a work unit in several rounds.

A cold tile's single work unit walks about ceil(rows / TA_BATCH) / sb (workgroup, commit)
segments in rounds of TB_SEGS = 2048, so more than one round takes rows > 2048 * 4096 * sb, sb
being the batches per pass-A commit of the plan; a unit holds at most
TB_ROUNDS * TB_THREADS = 6144 segments, which is three rounds.  Each row count is a round
figure just past its threshold that gives the wanted rounds at every pass-A occupancy.

name -> (plan of tile_plan_check's rounds mode, rows, rounds: an exact count, or None for >= 2)"""

BATCH = 4096          # TA_BATCH
N_SB3 = 6150 * BATCH  # 25.2 M rows: past 2048 * 4096 * 3
N_SB1 = 2100 * BATCH  # 8.6 M rows: past 2048 * 4096
N_SB1_CEIL = 4104 * BATCH        # sb = 1: between 4096 and 6144 segments per unit, three rounds
N_SB1_ODD = 2099 * BATCH + 1235  # sb = 1: two rounds; odd, no multiple of the batch or of any W

CASES = {
    "c2": ("c2", N_SB3, None),
    "mm_simple": ("mm_simple", N_SB3, None),
    "minmax": ("minmax", N_SB3, None),
    "two_slots_2d": ("2sum2d", N_SB1, None),
    "two_slots_3d": ("2sum3d", N_SB1_CEIL, 3),
    "var": ("var", N_SB3, None),
    "moment3": ("moment3", N_SB3, None),
    "f32": ("f32", N_SB3, None),
    "dense_f64": ("ord_f64", N_SB3, None),
    "dense_i8_f32": ("ord_i8f32", N_SB3, None),
    "dense_f64_filtered": ("ord_f64_mask", N_SB3, None),
    "odd_tail": ("2sum3d", N_SB1_ODD, None),
}
# pairs whose pass-A workgroups must differ in their commit counts (the tile table's empty tail rows)
TAIL_CASES = ("odd_tail",)
