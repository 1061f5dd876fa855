// prt_selection.hpp -- the selected rows of a sensitivity call: n_selected row numbers ordered by
// group, group g's being [group_first[g], group_first[g + 1]).  A pass checks its own buffers, then the selection here.
#pragma once

static int selection_check(const char* name, int64_t n_rows, int64_t n_selected, const int64_t* group_first, int n_groups,
                           int weight_column) {
  const char* bad = nullptr;
  if (n_selected > n_rows) bad = ": more selected rows than rows";
  else if (group_first[0] != 0 || group_first[n_groups] != n_selected) bad = ": group_first runs from 0 to n_selected";
  for (int g = 0; g < n_groups && !bad; ++g)
    if (group_first[g] > group_first[g + 1]) bad = ": group_first does not decrease";
  if (bad) return fail(PRT_ERR_ARG, std::string(name) + bad);
  if (weight_column < -1 || weight_column >= PRT_RECORD_COLS) return fail(PRT_ERR_ARG, "weight_column: 0..14 or -1");
  return PRT_OK;
}
