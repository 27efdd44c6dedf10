// Probe control law of the plant-plugin tests (tests/plant_plugin_cases.py) for the one input tests/control_probe.hip has no field
// for: the reference table as the law sees it.  The reward next to it is tests/plugin_probe.hip, which owns params[0], params[1].
//   params[2]  mode
//     0  column a of the step's table row, in.row[a] (PLPROBE_BAD without a table or for a >= table_cols)
//     1  in.row_index
//     2  in.table_rows      3  in.table_cols
//     4  column a of the table's LAST row read through in.table (the whole table for look-ahead); PLPROBE_BAD as in mode 0
#define PLPROBE_BAD (-12345.f)

DIAL_DEV float dial_user_control(const DialControlIn& in, int a, const float* params, const float* info_user) {
  (void)info_user;
  const int mode = (int)params[2];
  const bool has = in.row != nullptr && in.table != nullptr && a < in.table_cols;
  if (mode == 0) return has ? in.row[a] : PLPROBE_BAD;
  if (mode == 1) return (float)in.row_index;
  if (mode == 2) return (float)in.table_rows;
  if (mode == 3) return (float)in.table_cols;
  if (mode == 4) return has ? in.table[(size_t)(in.table_rows - 1) * in.table_cols + a] : PLPROBE_BAD;
  return PLPROBE_BAD;
}
