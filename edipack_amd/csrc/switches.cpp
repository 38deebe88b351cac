// switches.cpp -- the table of switches.hpp and the only readers of the environment in the library
#include "switches.hpp"

#include <algorithm>
#include <cstdlib>

namespace edigpu {

#define EDIGPU_SWITCH_ROW(field, type, name, rule, dflt, lo, hi, what) {name, SwitchRule::rule, dflt, lo, hi, EDIGPU_SWITCH_MOMENT, what},
#define EDIGPU_SWITCH_COUNT(field, type, name, rule, dflt, lo, hi, what) +1

static const SwitchRow kTable[] = {
#define EDIGPU_SWITCH_MOMENT SwitchMoment::SetUp
    EDIGPU_SETUP_SWITCHES(EDIGPU_SWITCH_ROW)
#undef EDIGPU_SWITCH_MOMENT
#define EDIGPU_SWITCH_MOMENT SwitchMoment::Comm
    EDIGPU_COMM_SWITCHES(EDIGPU_SWITCH_ROW)
#undef EDIGPU_SWITCH_MOMENT
#define EDIGPU_SWITCH_MOMENT SwitchMoment::Loop
    EDIGPU_LOOP_SWITCHES(EDIGPU_SWITCH_ROW)
#undef EDIGPU_SWITCH_MOMENT
};
constexpr int kSetupRows = 0 EDIGPU_SETUP_SWITCHES(EDIGPU_SWITCH_COUNT);
constexpr int kCommRows = 0 EDIGPU_COMM_SWITCHES(EDIGPU_SWITCH_COUNT);

const SwitchRow* switch_table(int* nrows) {
  *nrows = (int)(sizeof(kTable) / sizeof(kTable[0]));
  return kTable;
}

// e: the variable's text, not null for the ...OrUnset rules
static int64_t parse(const SwitchRow& r, const char* e) {
  switch (r.rule) {
    case SwitchRule::Present: return e != nullptr;
    case SwitchRule::FirstIsOne: return e && e[0] == '1';
    case SwitchRule::OnUnlessZero: return !e || atoi(e) != 0;
    case SwitchRule::OffUnlessNonzero: return e && atoi(e) != 0;
    case SwitchRule::Int: return e ? std::clamp<int64_t>(atoi(e), r.lo, r.hi) : r.dflt;
    case SwitchRule::Int64: return e ? std::clamp<int64_t>(atoll(e), r.lo, r.hi) : r.dflt;
    case SwitchRule::IntOrUnset: return atoi(e);
    case SwitchRule::Int64OrUnset: return atoll(e);
    case SwitchRule::DoubleOrUnset: break;
  }
  return 0;
}

template <class T>
static void read(T& field, const SwitchRow& r, const char* e) {
  field = (T)parse(r, e);
}
template <class T>
static void read(std::optional<T>& field, const SwitchRow& r, const char* e) {
  field = e ? std::optional<T>((T)parse(r, e)) : std::nullopt;
}
static void read(OptDouble& field, const SwitchRow&, const char* e) { field = e ? OptDouble(atof(e)) : std::nullopt; }

#define EDIGPU_SWITCH_READ(field, type, env_name, rule, dflt, lo, hi, what) \
  read(s.field, *row, getenv(env_name));                                    \
  row++;

Switches Switches::sample() {
  Switches s;
  const SwitchRow* row = kTable;
  EDIGPU_SETUP_SWITCHES(EDIGPU_SWITCH_READ)
  return s;
}

CommSwitches CommSwitches::sample() {
  CommSwitches s;
  const SwitchRow* row = kTable + kSetupRows;
  EDIGPU_COMM_SWITCHES(EDIGPU_SWITCH_READ)
  return s;
}

LoopSwitches LoopSwitches::sample() {
  LoopSwitches s;
  const SwitchRow* row = kTable + kSetupRows + kCommRows;
  EDIGPU_LOOP_SWITCHES(EDIGPU_SWITCH_READ)
  return s;
}

}  // namespace edigpu
