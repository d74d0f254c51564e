"""One-line mutants of csrc/smooth.hip and csrc/activity.hip and the cases that must notice each: the list
tests/test_track_mutants_native.py holds the two case lists to.

A mutant is (id, csrc file, old text, new text, killers).  `old text` occurs exactly once in the shipped file (the test asserts
it, so the list cannot rot when the kernels are edited); `killers` are names of smooth_cases.CASES / activity_cases.CASES, at
least one of which must fail `check` -- or be reported by a sanitizer -- on the host build of the mutated text.  The mutated text
exists in the test's temporary directory only: never in the tree, never in the library, never on a GPU.

The first block of each file are mutants that passed every case there was before the cases named here were added."""

SMOOTH, ACTIVITY = "smooth.hip", "activity.hip"

MUTANTS = [
    # ---- smooth.hip: survivors of the first 17 cases -------------------------------------------------------------------------
    ("fallback_c_0.005", SMOOTH, "kFallbackC = 0.05;", "kFallbackC = 0.005;", ["knife_c_below"]),
    ("fallback_c_0.5", SMOOTH, "kFallbackC = 0.05;", "kFallbackC = 0.5;", ["knife_c_above"]),
    ("fallback_c_0.045", SMOOTH, "kFallbackC = 0.05;", "kFallbackC = 0.045;", ["knife_c_below"]),
    ("fallback_c_0.055", SMOOTH, "kFallbackC = 0.05;", "kFallbackC = 0.055;", ["knife_c_above"]),
    ("weight_at_df_0", SMOOTH, "const double w = df == 0 ? 1.0 : exp(", "const double w = exp(", ["sigma_1e-200"]),
    ("radius_ceil_minus_1e-9", SMOOTH, "std::ceil(3.0 * sigma)", "std::ceil(3.0 * sigma - 1e-9)", ["sigma_1_up"]),
    ("radius_ceil_plus_1e-9", SMOOTH, "std::ceil(3.0 * sigma)", "std::ceil(3.0 * sigma + 1e-9)", ["sigma_1"]),
    ("radius_floor_plus_1", SMOOTH, "std::ceil(3.0 * sigma)", "(std::floor(3.0 * sigma) + 1.0)", ["sigma_1"]),
    ("tile_origin_rounded_down", SMOOTH, "const int a = p.row0 + (int)blockIdx.x * kTileRows,",
     "const int a = p.row0 / kTileRows * kTileRows + (int)blockIdx.x * kTileRows,", ["many_m2_s1.5", "many_m15_s5"]),
    ("second_tie_rule_to_the_larger_k", SMOOTH, "(cost == best_cost && df < best_df)", "(cost == best_cost && df <= best_df)",
     ["wild_m2_s1.5", "wild_m3_s0"]),
    ("nan_c_does_not_fall_back", SMOOTH, "if (!(c >= kFallbackC)) return false;", "if (c < kFallbackC) return false;",
     ["nonfinite_m0_s1.5", "nonfinite_m2_s1.5"]),
    # ---- smooth.hip: killed before ---------------------------------------------------------------------------------------------
    ("first_tie_rule_reversed", SMOOTH, "(cost == best_cost && df < best_df)", "(cost == best_cost && df > best_df)", ["short_m2_s1.5"]),
    # ---- activity.hip: survivors of the first 13 cases -------------------------------------------------------------------------
    ("rapid_needs_no_older_chunk", ACTIVITY, "need = c0 > k_first && (covered || i - c0 < R);", "need = c0 > k_first && covered;",
     ["lattice_H33_R33", "lattice_H64_R64", "lattice_H65_R33", "lattice_H96_R96", "lattice_H100_R50"]),
    ("whole_at_span_h_minus_g", ACTIVITY, "fi - f_prev > (long long)H - (long long)p.G", "fi - f_prev >= (long long)H - (long long)p.G",
     ["span_edge"]),
    ("spread_backwards_in_frames", ACTIVITY, "if (df >= 0 && df <= p.H) acc |= m[u];", "if (df <= p.H) acc |= m[u];", ["spread_back"]),
    # ---- activity.hip: killed before --------------------------------------------------------------------------------------------
    ("uncovered_lane_stops_at_once", ACTIVITY, "if (!covered && i - k > R) continue;", "if (!covered) continue;", ["wild_frames"]),
    ("in_r_without_its_row_bound", ACTIVITY, "const bool in_r = i - k <= R && df <= R;", "const bool in_r = df <= R;", ["wild_frames"]),
    ("negative_step_keeps_the_anchor", ACTIVITY, "step > p.G || step < 0;", "step > p.G;", ["wild_frames"]),
    ("spread_bound_h_minus_1", ACTIVITY, "const int e_hi = min(i + p.H, end - 1);", "const int e_hi = min(i + p.H - 1, end - 1);",
     ["still_segment"]),
    ("lowest_from_a_minus_h_plus_1", ACTIVITY, "const int lowest = max(a - H, first_s[0]);", "const int lowest = max(a - H + 1, first_s[0]);",
     ["many_tracks"]),
]
IDS = [m[0] for m in MUTANTS]


def mutate(text, old, new):
    """-> the text with its one occurrence of `old` replaced; asserts that there is exactly one."""
    assert text.count(old) == 1, f"{old!r} occurs {text.count(old)} times in the shipped file, not once: the mutant list has rotted"
    return text.replace(old, new)
