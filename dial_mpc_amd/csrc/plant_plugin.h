// plant_plugin.h -- the plant simulator of a task plugin (dial_plant_step on a dial_create_plugin context): plant_kernel.h's kernel at
// ONE model's compile-time dimensions, with the plugin's user control law (user_control.h) as a third control mode.  A plugin built
// with -DDIAL_PLUGIN_PLANT=1 (dial_mpc_amd/plugin.py: build_plugin(plant=True)) instantiates plant_kernel at its Dims and exports a
// FOURTH optional table under a symbol of its own; dial_plugin_ops, dial_plugin_ctrl, dial_plugin_table and their versions stay as
// they are, and a plugin built without the flag carries neither the kernel nor the symbol (dial_plant_step then refuses its
// contexts).  This header holds the table only -- the kernel, its contract and its launch wrapper are plant_kernel.h's -- and
// libdialhip.so includes it for the table's layout: it instantiates no kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "plant_kernel.h"

#ifndef DIAL_PLUGIN_PLANT_VERSION   // (overridable on a plugin's command line: the tests build one that reports another version)
#define DIAL_PLUGIN_PLANT_VERSION 1
#endif
#define DIAL_PLUGIN_PLANT_SYMBOL "dial_plugin_plant_v1"
struct dial_plugin_plant {
  int version;                     // DIAL_PLUGIN_PLANT_VERSION
  int nq, nv, nu;                  // of the instantiation (the row strides of the launch below)
  size_t cmodel_bytes;             // sizeof(CModel<D>): the same constants as dial_plugin_ops' (ABI check)
  size_t sizeof_control_in;        // sizeof(DialControlIn)
  int has_law;                     // the plugin carries a user control law: DIAL_PLANT_LAW is available
  dial_plant_launch_fn launch;     // plant_kernel.h's launch signature; lds = the env.step workspace of the context
};
typedef const dial_plugin_plant* (*dial_plugin_plant_entry)(void);

// the table of one instantiation D: plant_kernel.h's launch wrapper, as libdialplant.so's table holds it for the built-in families
template <class D>
struct PluginPlant {
  static_assert(D::user && D::NU <= 64, "a task plugin's instantiation; one lane per actuator");
  static const dial_plugin_plant* table() {
    static const dial_plugin_plant tab = {DIAL_PLUGIN_PLANT_VERSION, D::NQ, D::NV, D::NU, sizeof(CModel<D>), sizeof(DialControlIn),
                                          D::user_ctrl ? 1 : 0, &plant_launch<D>};
    return &tab;
  }
};
