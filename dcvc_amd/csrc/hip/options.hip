// The option table behind dcvc_set_option / dcvc_get_option (options.h).
#include "options.h"

#include <cstring>
#include <vector>

#include "../../../include/dcvc_hip.h"

namespace {

struct Option {
  const char *name;
  int *value;
  int def;
};

// function-local: filled by static registrars of other translation units,
// whichever of them the loader initialises first
std::vector<Option> &registry() {
  static std::vector<Option> r;
  return r;
}

const Option *find(const char *name) {
  if (!name) return nullptr;
  for (const Option &o : registry())
    if (std::strcmp(o.name, name) == 0) return &o;
  return nullptr;
}

}  // namespace

DcvcOptionReg::DcvcOptionReg(const char *name, int *value, int def) { registry().push_back({name, value, def}); }

extern "C" int dcvc_set_option(const char *name, int value) {
  const Option *o = find(name);
  if (!o) return DCVC_HIP_EINVAL;
  *o->value = value;
  return DCVC_HIP_OK;
}

extern "C" int dcvc_get_option(const char *name, int *value) {
  const Option *o = find(name);
  if (!o || !value) return DCVC_HIP_EINVAL;
  *value = *o->value;
  return DCVC_HIP_OK;
}
