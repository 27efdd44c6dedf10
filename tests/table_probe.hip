// Probe reward of the reference-table tests (tests/table_cases.py): returns ONE value of what the reward sees of the table
// (csrc/user_reward.h), chosen at run time by (params[0], params[1]) = (field, index), so that one plugin per model serves every check.
//   field:  1 row[index]  2 table[index] (flat, read from global memory)  3 row_index  4 table_rows  5 table_cols
//   With no table bound (row == nullptr) every field returns TPROBE_NONE -- after checking that the other table fields are the
//   contract's null / zero values (TPROBE_BAD otherwise).  An index outside its array, or an unknown field, returns TPROBE_BAD (the
//   probe reads nothing out of bounds).
#define TPROBE_NONE (-777.f)
#define TPROBE_BAD (-12345.f)

DIAL_DEV float dial_user_reward(const DialRewardIn& in, const float* params, float* info_user) {
  (void)info_user;
  const int field = (int)params[0], i = (int)params[1];
  if (in.row == nullptr) return in.table == nullptr && in.table_rows == 0 && in.table_cols == 0 && in.row_index == 0 ? TPROBE_NONE : TPROBE_BAD;
  switch (field) {
    case 1: return i >= 0 && i < in.table_cols ? in.row[i] : TPROBE_BAD;
    case 2: return i >= 0 && i < in.table_rows * in.table_cols ? in.table[i] : TPROBE_BAD;
    case 3: return (float)in.row_index;
    case 4: return (float)in.table_rows;
    case 5: return (float)in.table_cols;
    default: return TPROBE_BAD;
  }
}
