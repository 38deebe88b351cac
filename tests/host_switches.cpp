// CPU shim for tests/test_switches.py: the table of environment switches (csrc/switches.hpp) and its three snapshots.
// Two slots per snapshot, so that a test can take one, change the environment and take another.
#include <cstring>

#include "host_sb.hpp"
#include "switches.hpp"

using namespace edigpu;

static Switches g_setup[2];
static CommSwitches g_comm[2];
static LoopSwitches g_loop[2];

static double num(bool v) { return v ? 1.0 : 0.0; }
static double num(int v) { return (double)v; }
static double num(int64_t v) { return (double)v; }
template <class T>
static double num(const std::optional<T>& v) { return (double)*v; }
template <class T>
static bool has(const T&) { return true; }
template <class T>
static bool has(const std::optional<T>& v) { return v.has_value(); }

extern "C" {

int sw_count() {
  int n = 0;
  switch_table(&n);
  return n;
}
static const SwitchRow& row(int i) {
  int n = 0;
  return switch_table(&n)[i];
}
const char* sw_name(int i) { return row(i).name; }
const char* sw_what(int i) { return row(i).what; }
int sw_rule(int i) { return (int)row(i).rule; }
int sw_moment(int i) { return (int)row(i).moment; }
long long sw_default(int i) { return row(i).dflt; }
long long sw_lo(int i) { return row(i).lo; }
long long sw_hi(int i) { return row(i).hi; }

void sw_take_setup(int slot) { g_setup[slot] = Switches::sample(); }
void sw_take_comm(int slot) { g_comm[slot] = CommSwitches::sample(); }
void sw_take_loop(int slot) { g_loop[slot] = LoopSwitches::sample(); }

// the value of the named switch in the slot's snapshot of its moment: 1 and *value; 0: a switch without a value (unset,
// derived default); -1: no such switch
int sw_get(int slot, const char* switch_name, double* value) {
#define EDIGPU_SWITCH_GET(field, type, name, rule, dflt, lo, hi, what) \
  if (!std::strcmp(switch_name, name)) {                               \
    if (!has(snap.field)) return 0;                                    \
    *value = num(snap.field);                                          \
    return 1;                                                          \
  }
  {
    const Switches& snap = g_setup[slot];
    EDIGPU_SETUP_SWITCHES(EDIGPU_SWITCH_GET)
  }
  {
    const CommSwitches& snap = g_comm[slot];
    EDIGPU_COMM_SWITCHES(EDIGPU_SWITCH_GET)
  }
  {
    const LoopSwitches& snap = g_loop[slot];
    EDIGPU_LOOP_SWITCHES(EDIGPU_SWITCH_GET)
  }
#undef EDIGPU_SWITCH_GET
  return -1;
}

// what set-up derives from the snapshot
long long sw_ib_min_row_bytes(int slot) { return g_setup[slot].ib_min_row_bytes(); }
int sw_blocked_shift(int slot) { return g_setup[slot].blocked_shift(); }
int sw_sb_cols_gs(int slot) { return sb_cols_gs(g_setup[slot].sb_cw); }

}  // extern "C"
