// What k_raycast.hip and k_raycast_sensors.hip share: the hull geometry tables as rayBodyCollider's Hull argument.
#pragma once
#include "mi_common.h"

struct RcHulls
{
	const float4* verts; const uint4* tris; const uint2* range;
	MI_DEV u32 numTriangles(u32 g) const { return range[g].y; }
	MI_DEV V3 vertex(u32 g, u32 f, u32 k) const { uint4 t = tris[range[g].x + f]; return v3f4(verts[k == 0 ? t.x : (k == 1 ? t.y : t.z)]); }
};
