// The launch menu's one definition site (menu.h): the process menu, read from the environment once at library load, and the C ABI
// that writes and reads it by key.
#include <stdlib.h>

#include "common.h"
#include "../../include/gget.h"

namespace {
LaunchMenu load_menu() {
  LaunchMenu m;
  for (const MenuRow& r : kMenuRows) {
    const char* e = r.env ? getenv(r.env) : nullptr;
    m.*r.field = e ? (r.env_presence ? 1 : atoi(e)) : r.def;
  }
  return m;
}
const MenuRow* find_key(int key) {
  for (const MenuRow& r : kMenuRows)
    if (key != 0 && r.key == key) return &r;
  gget_set_error("debug_set / debug_get: unknown key %d", key);
  return nullptr;
}
}  // namespace

LaunchMenu g_menu = load_menu();
thread_local const LaunchMenu* t_call_menu = nullptr;

extern "C" int gget_debug_set(int key, int value) {
  const MenuRow* r = find_key(key);
  if (!r) return 2;
  g_menu.*r->field = value;
  return 0;
}
extern "C" int gget_debug_get(int key, int* value) {
  GGET_REQUIRE(value != nullptr, "debug_get: null argument");
  const MenuRow* r = find_key(key);
  if (!r) return 2;
  *value = g_menu.*r->field;
  return 0;
}
