// What k_raycast.hip, k_raycast_sensors.hip and k_proximity.hip share: the hull geometry tables as rayBodyCollider's Hull argument,
// the layout of the tree k_raycast.hip builds in World::rc*, and the host function that builds it.
#pragma once
#include "mi_common.h"

struct RcHulls
{
	const float4* verts; const uint4* tris; const uint2* range;
	MI_DEV u32 numTriangles(u32 g) const { return range[g].y; }
	MI_DEV V3 vertex(u32 g, u32 f, u32 k) const { uint4 t = tris[range[g].x + f]; return v3f4(verts[k == 0 ? t.x : (k == 1 ? t.y : t.z)]); }
};

// ---- header words of World::rcCount (zeroed before every build; every accumulated word has 0 as its neutral element) ----
enum
{
	RC_N = 0,        // candidates
	RC_NEG_MIN = 1,  // 3 words: max of rcOrdered(-centre): the lower bound of the box centres
	RC_MAX = 4,      // 3 words: max of rcOrdered(centre)
	RC_DIAG = 7,     // float bits: largest diagonal of a padded leaf box
	RC_ABS = 8,      // float bits: largest |coordinate| of a padded leaf box
	RC_HEADER = 16,  // the arrival counters of the internal nodes follow
};
#define RC_LEAF 0x80000000u
#define RC_NO_PARENT 0xFFFFFFFFu
#define RC_NOT_A_CANDIDATE (1u << 30)
#define RC_KEY_BITS 30
// Depth of the tree = length of the longest chain of internal nodes.  Going down, the length of the common prefix of a node's range
// grows strictly; the prefix is counted over the 30 key bits and then, for equal keys, over the 32 bits of the sorted position.  The
// root's range has a prefix of >= 0 key bits and a node with two different leaves one of <= 61, so a chain has <= 62 nodes, and
// the stack, which holds one pending sibling per node of the chain, <= 62 entries.
#define RC_STACK 64
static_assert(RC_KEY_BITS + 32 <= RC_STACK, "k_raycast's stack holds one entry per level of the tree: key bits + position bits");
#define RC_EPS 1.1920929e-7f
#define RC_NODE_WORDS 16u // one internal node: 64 bytes (k_raycast.hip describes the record)
