// Private to the translation units of the C-ABI (api.hip, api_scene.hip, snapshot.hip): the handle behind mi_world* and its entry checks.
#pragma once
#include "world.h"

struct mi_world { World w; mi_world(int dev) : w(dev) {} };
#define W (&world->w)
#define CHECK_WORLD(ret) if (!world) return ret; g_currentWorld = W

extern thread_local std::string g_createError; // mi_last_error(NULL): why mi_world_create / mi_world_restore returned NULL (world.hip)
