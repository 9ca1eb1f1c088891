// The runtime switches of libdcvc_hip (dcvc_set_option / dcvc_get_option).
//
// An option is one plain int, declared once, beside the code that reads it:
//   DCVC_OPTION("dconv_bn128", g_bn128, 1);   // what 0 / 1 / n mean
// defines `int g_bn128 = 1` and registers it under its name when the library
// is loaded.  The comment beside the declaration is the option's
// documentation.  Launchers read the int; the name is only looked up by
// dcvc_set_option / dcvc_get_option.  Registration touches no HIP runtime, so
// the library still loads (and its options can be set) on a host without a GPU.
#pragma once

struct DcvcOptionReg {
  DcvcOptionReg(const char *name, int *value, int def);
};

#define DCVC_OPTION(name, var, def) \
  int var = def;                    \
  static const DcvcOptionReg var##_option(name, &var, def)
