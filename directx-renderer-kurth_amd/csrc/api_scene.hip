// C-ABI of include/mi_physics.h, part 1: what a world is made of — bodies, colliders and hull geometries, force fields and triggers
// (with the event drain), the heightmap terrain, cloths, and the constraints.  A thin shell over World's host mirrors.
#include "api.h"
#include <cstring>
#include <cmath>
#include <algorithm>

extern "C" {

uint32_t mi_add_body(mi_world* world, int kinematic, float gravityFactor, float linearDamping, float angularDamping, const float pos[3], const float rot[4])
{
	CHECK_WORLD(0xFFFFFFFFu);
	World::HBody b{};
	memcpy(b.pos, pos, 12); memcpy(b.rot, rot, 16);
	if (kinematic) { b.invMass = 0.f; }                                   // rigid_body.cpp:8-17
	else { b.invMass = 1.f; b.invInertia[0] = b.invInertia[4] = b.invInertia[8] = 1.f; }
	b.gravityFactor = gravityFactor; b.linDamp = linearDamping; b.angDamp = angularDamping;
	W->bodies.push_back(b);
	W->topologyDirty = true;
	return (uint32_t)W->bodies.size() - 1;
}

static uint32_t addCollider(World* w, uint32_t body, uint32_t type, const float* shape, const mi_material* material, const float* pos, const float* rot)
{
	if (type > MI_HULL) { w->fail(MI_ERR_INVALID_ARGUMENT, "mi_add_collider: unknown collider type"); return 0xFFFFFFFFu; }
	if (type == MI_HULL && (shape[7] < 0.f || (size_t)shape[7] >= w->hulls.size())) { w->fail(MI_ERR_INVALID_ARGUMENT, "mi_add_collider: hull geometry index out of range (mi_add_hull_geometry first)"); return 0xFFFFFFFFu; }
	if (body != MI_STATIC_BODY && body >= w->bodies.size()) { w->fail(MI_ERR_INVALID_ARGUMENT, "mi_add_collider: body out of range"); return 0xFFFFFFFFu; }
	World::HCollider c; memset(&c, 0, sizeof(c));
	u32 n = (type == MI_SPHERE) ? 4 : ((type == MI_CAPSULE || type == MI_CYLINDER) ? 7 : (type == MI_AABB ? 6 : (type == MI_HULL ? 8 : 10)));
	memcpy(c.shape, shape, n * sizeof(float));
	c.restitution = material->restitution; c.friction = material->friction; c.density = material->density;
	c.type = type; c.body = body;
	if (pos) memcpy(c.spos, pos, 12);
	if (rot) memcpy(c.srot, rot, 16); else c.srot[3] = 1.f;
	u32 id = (u32)w->colliders.size();
	w->colliders.push_back(c);
	if (body != MI_STATIC_BODY)
	{
		if (w->stateOnDevice) w->downloadState();
		w->bodies[body].colliders.push_back(id);
		recalculateProperties(*w, w->bodies[body]);                      // scene.h:60-63
	}
	w->topologyDirty = true;
	return id;
}
uint32_t mi_add_hull_geometry(mi_world* world, const float* vertices3, uint32_t numVertices, const uint32_t* triangles3, uint32_t numTriangles)
{
	CHECK_WORLD(0xFFFFFFFFu);
	if (!vertices3 || !triangles3 || numVertices < 4 || numTriangles < 4) { W->fail(MI_ERR_INVALID_ARGUMENT, "mi_add_hull_geometry: a convex hull needs at least 4 vertices and 4 triangles"); return 0xFFFFFFFFu; }
	World::HHull g;
	g.vertices.assign(vertices3, vertices3 + 3 * (size_t)numVertices);
	g.triangles.assign(triangles3, triangles3 + 3 * (size_t)numTriangles);
	for (uint32_t t = 0; t < 3 * numTriangles; ++t) if (triangles3[t] >= numVertices) { W->fail(MI_ERR_INVALID_ARGUMENT, "mi_add_hull_geometry: triangle index out of range"); return 0xFFFFFFFFu; }
	for (int k = 0; k < 3; ++k) { g.aabbMin[k] = MI_FLT_MAX; g.aabbMax[k] = -MI_FLT_MAX; }
	for (uint32_t v = 0; v < numVertices; ++v) for (int k = 0; k < 3; ++k) { g.aabbMin[k] = fminf(g.aabbMin[k], vertices3[3 * v + k]); g.aabbMax[k] = fmaxf(g.aabbMax[k], vertices3[3 * v + k]); }
	W->hulls.push_back(g);
	W->topologyDirty = true;
	return (uint32_t)W->hulls.size() - 1;
}

uint32_t mi_add_collider(mi_world* world, uint32_t body, uint32_t type, const float* shape, const mi_material* material)
{
	CHECK_WORLD(0xFFFFFFFFu);
	return addCollider(W, body, type, shape, material, nullptr, nullptr);
}
uint32_t mi_add_static_collider(mi_world* world, uint32_t type, const float* shape, const mi_material* material, const float pos[3], const float rot[4])
{
	CHECK_WORLD(0xFFFFFFFFu);
	return addCollider(W, MI_STATIC_BODY, type, shape, material, pos, rot);
}

// ---- force fields, triggers, events (physics.h:182-203, 356-380; physics.cpp:759-787, 952-1178) ----
static void setPose(float* pos, float* rot, const float* p, const float* r)
{
	pos[0] = pos[1] = pos[2] = 0.f; rot[0] = rot[1] = rot[2] = 0.f; rot[3] = 1.f;
	if (p) memcpy(pos, p, 12);
	if (r) memcpy(rot, r, 16);
}
uint32_t mi_add_force_field(mi_world* world, const float force[3], const float pos[3], const float rot[4])
{
	CHECK_WORLD(0xFFFFFFFFu);
	if (!force) { W->fail(MI_ERR_INVALID_ARGUMENT, "mi_add_force_field: force is NULL"); return 0xFFFFFFFFu; }
	if (W->zones.fields.size() >= (1u << 24)) { W->fail(MI_ERR_CAPACITY, "mi_add_force_field: too many fields"); return 0xFFFFFFFFu; }
	World::HField f; memset(&f, 0, sizeof(f));
	memcpy(f.force, force, 12); setPose(f.pos, f.rot, pos, rot); f.hasTransform = (pos || rot) ? 1u : 0u;
	W->zones.fields.push_back(f); W->zones.fieldsDirty = true;
	return (uint32_t)W->zones.fields.size() - 1;
}
int mi_set_force_field(mi_world* world, uint32_t field, const float force[3])
{
	CHECK_WORLD(MI_ERR_INVALID_ARGUMENT);
	if (field >= W->zones.fields.size() || !force) { W->fail(MI_ERR_INVALID_ARGUMENT, "mi_set_force_field: field out of range"); return W->lastError; }
	memcpy(W->zones.fields[field].force, force, 12); W->zones.fieldsDirty = true;
	return MI_OK;
}
uint32_t mi_add_trigger(mi_world* world, const float pos[3], const float rot[4])
{
	CHECK_WORLD(0xFFFFFFFFu);
	if (W->zones.triggers.size() >= (1u << 24)) { W->fail(MI_ERR_CAPACITY, "mi_add_trigger: too many triggers"); return 0xFFFFFFFFu; }
	World::HTrigger t; memset(&t, 0, sizeof(t)); setPose(t.pos, t.rot, pos, rot);
	W->zones.triggers.push_back(t);
	return (uint32_t)W->zones.triggers.size() - 1;
}
static uint32_t addZoneCollider(World* w, u32 zoneType, u32 zoneIndex, const float* pos, const float* rot, uint32_t type, const float* shape)
{
	mi_material none = { 0.f, 0.f, 0.f };
	uint32_t id = addCollider(w, MI_STATIC_BODY, type, shape, &none, pos, rot);
	if (id != 0xFFFFFFFFu) { w->colliders[id].zoneType = zoneType; w->colliders[id].zoneIndex = zoneIndex; }
	return id;
}
uint32_t mi_add_force_field_collider(mi_world* world, uint32_t field, uint32_t type, const float* shape)
{
	CHECK_WORLD(0xFFFFFFFFu);
	if (field >= W->zones.fields.size() || !shape) { W->fail(MI_ERR_INVALID_ARGUMENT, "mi_add_force_field_collider: field out of range"); return 0xFFFFFFFFu; }
	World::HField& f = W->zones.fields[field];
	uint32_t id = addZoneCollider(W, 2u, field, f.pos, f.rot, type, shape);
	if (id != 0xFFFFFFFFu) { f.numColliders++; W->zones.fieldsDirty = true; }
	return id;
}
uint32_t mi_add_trigger_collider(mi_world* world, uint32_t trigger, uint32_t type, const float* shape)
{
	CHECK_WORLD(0xFFFFFFFFu);
	if (trigger >= W->zones.triggers.size() || !shape) { W->fail(MI_ERR_INVALID_ARGUMENT, "mi_add_trigger_collider: trigger out of range"); return 0xFFFFFFFFu; }
	World::HTrigger& t = W->zones.triggers[trigger];
	uint32_t id = addZoneCollider(W, 3u, trigger, t.pos, t.rot, type, shape);
	if (id != 0xFFFFFFFFu) t.numColliders++;
	return id;
}
static int moveZone(World* w, u32 zoneType, u32 zoneIndex, float* zpos, float* zrot, const float* pos, const float* rot)
{
	if (!pos || !rot) { w->fail(MI_ERR_INVALID_ARGUMENT, "zone transform: pos / rot is NULL"); return w->lastError; }
	memcpy(zpos, pos, 12); memcpy(zrot, rot, 16);
	for (u32 i = 0; i < (u32)w->colliders.size(); ++i)
	{
		World::HCollider& c = w->colliders[i];
		if (c.zoneType != zoneType || c.zoneIndex != zoneIndex) continue;
		memcpy(c.spos, pos, 12); memcpy(c.srot, rot, 16);
		if (!w->topologyDirty && i < w->nc) // the collider is on the device already: patch its static pose in place
		{
			float4 sp[2] = { make_float4(pos[0], pos[1], pos[2], 0.f), make_float4(rot[0], rot[1], rot[2], rot[3]) };
			MI_CHECK(hipMemcpyAsync(w->colStaticPose.p + 2 * (size_t)i, sp, sizeof(sp), hipMemcpyHostToDevice, w->stream));
			MI_CHECK(hipStreamSynchronize(w->stream));
		}
	}
	return w->lastError;
}
int mi_set_force_field_transform(mi_world* world, uint32_t field, const float pos[3], const float rot[4])
{
	CHECK_WORLD(MI_ERR_INVALID_ARGUMENT);
	if (field >= W->zones.fields.size()) { W->fail(MI_ERR_INVALID_ARGUMENT, "mi_set_force_field_transform: field out of range"); return W->lastError; }
	W->zones.fields[field].hasTransform = 1u; W->zones.fieldsDirty = true;
	return moveZone(W, 2u, field, W->zones.fields[field].pos, W->zones.fields[field].rot, pos, rot);
}
int mi_set_trigger_transform(mi_world* world, uint32_t trigger, const float pos[3], const float rot[4])
{
	CHECK_WORLD(MI_ERR_INVALID_ARGUMENT);
	if (trigger >= W->zones.triggers.size()) { W->fail(MI_ERR_INVALID_ARGUMENT, "mi_set_trigger_transform: trigger out of range"); return W->lastError; }
	return moveZone(W, 3u, trigger, W->zones.triggers[trigger].pos, W->zones.triggers[trigger].rot, pos, rot);
}
int mi_enable_collision_events(mi_world* world, int begin, int end)
{
	CHECK_WORLD(MI_ERR_INVALID_ARGUMENT);
	W->zones.collisionBeginEvents = begin != 0; W->zones.collisionEndEvents = end != 0;
	return MI_OK;
}
uint32_t mi_drain_events(mi_world* world, mi_event* out, uint32_t capacity)
{
	CHECK_WORLD(0);
	if (W->zones.eventRing.p)
	{
		u32 head[2] = { 0, 0 };
		MI_CHECK(hipMemcpyAsync(head, W->dCounters.p + CTR_EVENT_COUNT, sizeof(head), hipMemcpyDeviceToHost, W->stream));
		MI_CHECK(hipStreamSynchronize(W->stream));
		u32 n = std::min(head[0], W->zones.eventCap);
		if (n)
		{
			size_t first = W->zones.pendingEvents.size();
			W->zones.pendingEvents.resize(first + n);
			MI_CHECK(hipMemcpyAsync(W->zones.pendingEvents.data() + first, W->zones.eventRing.p, sizeof(mi_event) * n, hipMemcpyDeviceToHost, W->stream));
			MI_CHECK(hipStreamSynchronize(W->stream));
			// the order the reference's merge loops call back in: per step the trigger events, then the collision events, each by pair
			std::sort(W->zones.pendingEvents.begin() + first, W->zones.pendingEvents.end(), [](const mi_event& x, const mi_event& y)
			{
				if (x.step != y.step) return x.step < y.step;
				u32 cx = x.kind >> 1, cy = y.kind >> 1;
				if (cx != cy) return cx < cy;
				if (x.a != y.a) return x.a < y.a;
				return x.b < y.b;
			});
		}
		if (head[0] || head[1]) MI_CHECK(hipMemsetAsync(W->dCounters.p + CTR_EVENT_COUNT, 0, sizeof(head), W->stream));
		if (head[1] & 1u) W->fail(MI_ERR_CAPACITY, "the event ring overflowed: events were lost (drain more often or raise MI_EVENT_CAPACITY)");
		if (head[1] & 2u) W->fail(MI_ERR_CAPACITY, "a trigger / collision overlap set was full: events were lost");
	}
	uint32_t n = (uint32_t)std::min<size_t>(capacity, W->zones.pendingEvents.size());
	if (n && out) memcpy(out, W->zones.pendingEvents.data(), sizeof(mi_event) * n);
	W->zones.pendingEvents.erase(W->zones.pendingEvents.begin(), W->zones.pendingEvents.begin() + n);
	return n;
}

// ---- heightmap terrain (heightmap_collider.h:127-152, heightmap_collider.cpp:5-38) ----
int mi_set_heightmap(mi_world* world, uint32_t chunksPerDim, float chunkSize, const mi_material* material, const float minCorner[3], float amplitudeScale)
{
	CHECK_WORLD(MI_ERR_INVALID_ARGUMENT);
	if (!chunksPerDim || chunksPerDim > 256 || !(chunkSize > 0.f) || !(amplitudeScale > 0.f) || !material || !minCorner) { W->fail(MI_ERR_INVALID_ARGUMENT, "mi_set_heightmap: 1..256 chunks per dimension, positive chunk size and amplitude"); return W->lastError; }
	W->resolvePendingFlow();
	W->terrain.chunksPerDim = chunksPerDim; W->terrain.chunkSize = chunkSize; W->terrain.amplitude = amplitudeScale;
	memcpy(W->terrain.minCorner, minCorner, 12); W->terrain.material[0] = material->restitution; W->terrain.material[1] = material->friction; W->terrain.material[2] = material->density;
	size_t chunks = (size_t)chunksPerDim * chunksPerDim;
	W->terrain.hHeights.assign(chunks * 129 * 129, 0); W->terrain.hValid.assign(chunks, 0);
	W->queries.terrainTableValid = false;
	W->terrain.heights.ensure(W->terrain.hHeights.size(), W->stream); W->terrain.valid.ensure(chunks, W->stream);
	MI_CHECK(hipMemsetAsync(W->terrain.valid.p, 0, sizeof(u32) * chunks, W->stream));
	if (const char* e = getenv("MI_TERRAIN_SLOTS_PER_COLLIDER")) W->terrain.slotsPerCollider = (u32)std::max(1, atoi(e));
	if (const char* e = getenv("MI_TERRAIN_MIN_SLOTS")) W->terrain.minSlots = (u32)std::max(1, atoi(e));
	return W->lastError;
}
int mi_heightmap_set_chunk(mi_world* world, uint32_t x, uint32_t z, const uint16_t* heights129x129) // heightmap_collider_chunk::setHeights
{
	CHECK_WORLD(MI_ERR_INVALID_ARGUMENT);
	if (!W->terrain.chunksPerDim || x >= W->terrain.chunksPerDim || z >= W->terrain.chunksPerDim || !heights129x129) { W->fail(MI_ERR_INVALID_ARGUMENT, "mi_heightmap_set_chunk: chunk out of range (mi_set_heightmap first)"); return W->lastError; }
	W->resolvePendingFlow();
	size_t chunk = (size_t)z * W->terrain.chunksPerDim + x, n = 129 * 129;
	memcpy(W->terrain.hHeights.data() + chunk * n, heights129x129, sizeof(uint16_t) * n);
	W->terrain.hValid[chunk] = 1;
	W->queries.terrainTableValid = false;
	MI_CHECK(hipMemcpyAsync(W->terrain.heights.p + chunk * n, W->terrain.hHeights.data() + chunk * n, sizeof(uint16_t) * n, hipMemcpyHostToDevice, W->stream));
	MI_CHECK(hipMemcpyAsync(W->terrain.valid.p + chunk, W->terrain.hValid.data() + chunk, sizeof(u32), hipMemcpyHostToDevice, W->stream));
	MI_CHECK(hipStreamSynchronize(W->stream));
	return W->lastError;
}
int mi_heightmap_update(mi_world* world, const float minCorner[3], float amplitudeScale) // heightmap_collider_component::update
{
	CHECK_WORLD(MI_ERR_INVALID_ARGUMENT);
	if (!W->terrain.chunksPerDim || !minCorner || !(amplitudeScale > 0.f)) { W->fail(MI_ERR_INVALID_ARGUMENT, "mi_heightmap_update: no heightmap, or amplitude not positive"); return W->lastError; }
	memcpy(W->terrain.minCorner, minCorner, 12); W->terrain.amplitude = amplitudeScale;
	return MI_OK;
}
float mi_heightmap_height_at(mi_world* world, float wx, float wz) // heightmap_collider_component::getHeightAt: -FLT_MAX outside the terrain
{
	CHECK_WORLD(-MI_FLT_MAX);
	if (!W->terrain.chunksPerDim) return -MI_FLT_MAX;
	float invChunkSize = 1.f / W->terrain.chunkSize, heightScale = W->terrain.amplitude / 65535;
	float cx = (wx - W->terrain.minCorner[0]) * invChunkSize, cz = (wz - W->terrain.minCorner[2]) * invChunkSize;
	if (cx < 0.f || cz < 0.f || cx >= W->terrain.chunksPerDim || cz >= W->terrain.chunksPerDim) return -MI_FLT_MAX;
	u32 chunk = (u32)cz * W->terrain.chunksPerDim + (u32)cx;
	if (!W->terrain.hValid[chunk]) return -MI_FLT_MAX;
	cx = fmodf(cx, 1.f) * 128; cz = fmodf(cz, 1.f) * 128;
	u32 x = (u32)cx, z = (u32)cz;
	float relX = cx - x, relZ = cz - z;
	const uint16_t* H = W->terrain.hHeights.data() + (size_t)chunk * 129 * 129;
	float a = H[129 * z + x] * heightScale, b = H[129 * (z + 1) + x] * heightScale, c = H[129 * z + x + 1] * heightScale, d = H[129 * (z + 1) + x + 1] * heightScale;
	float l0 = a + relX * (c - a), l1 = b + relX * (d - b);
	return (l0 + relZ * (l1 - l0)) + W->terrain.minCorner[1];
}

// ---- cloth (cloth.h:5-60) ----
static V3 clothParticlePosition(const World::HCloth& c, float relX, float relY) // cloth.cpp:134-140
{
	V3 position = v3(relX * c.width, -relY * c.height, 0.f);
	position.x -= c.width * 0.5f;
	float t = position.y; position.y = position.z; position.z = t;
	return position;
}
uint32_t mi_add_cloth(mi_world* world, float width, float height, uint32_t gridSizeX, uint32_t gridSizeY, float totalMass, float stiffness, float damping, float gravityFactor)
{
	CHECK_WORLD(0xFFFFFFFFu);
	if (gridSizeX < 2 || gridSizeY < 2 || (uint64_t)gridSizeX * gridSizeY > (1u << 24) || !(totalMass > 0.f) || !(stiffness > 0.f))
	{ W->fail(MI_ERR_INVALID_ARGUMENT, "mi_add_cloth: needs a grid of at least 2 x 2 particles, positive mass and stiffness"); return 0xFFFFFFFFu; }
	W->downloadCloths();
	World::HCloth c;
	c.width = width; c.height = height; c.totalMass = totalMass; c.stiffness = stiffness; c.damping = damping; c.gravityFactor = gravityFactor;
	c.oldTotalMass = totalMass; c.oldStiffness = stiffness; c.gridX = gridSizeX; c.gridY = gridSizeY;
	u32 n = gridSizeX * gridSizeY;
	float invMassPerParticle = n / totalMass;
	c.pos.resize(3 * (size_t)n); c.vel.assign(3 * (size_t)n, 0.f); c.invMass.resize(n);
	for (u32 y = 0; y < gridSizeY; ++y)
		for (u32 x = 0; x < gridSizeX; ++x)
		{
			V3 p = clothParticlePosition(c, x / (float)(gridSizeX - 1), y / (float)(gridSizeY - 1));
			u32 i = y * gridSizeX + x;
			c.pos[3 * i] = p.x; c.pos[3 * i + 1] = p.y; c.pos[3 * i + 2] = p.z;
			c.invMass[i] = (y == 0) ? 0.f : invMassPerParticle; // the upper row is locked (cloth.cpp:29)
		}
	c.prev = c.pos;
	auto add = [&c](u32 a, u32 b, u32 color) // cloth.cpp:320-329
	{
		V3 d = v3(c.pos[3 * a] - c.pos[3 * b], c.pos[3 * a + 1] - c.pos[3 * b + 1], c.pos[3 * a + 2] - c.pos[3 * b + 2]);
		c.constraints.push_back(World::HClothConstraint{ a, b, length(d), (c.invMass[a] + c.invMass[b]) / c.stiffness, color });
	};
	for (u32 y = 0; y < gridSizeY; ++y) // cloth.cpp:46-84; colour = constraint family x one parity bit (no two constraints of a colour share a particle)
		for (u32 x = 0; x < gridSizeX; ++x)
		{
			u32 index = y * gridSizeX + x;
			if (x + 1 < gridSizeX) add(index, index + 1, 0 + (x & 1));
			if (y + 1 < gridSizeY) add(index, index + gridSizeX, 2 + (y & 1));
			if (x + 1 < gridSizeX && y + 1 < gridSizeY) { add(index, index + gridSizeX + 1, 4 + (x & 1)); add(index + gridSizeX, index + 1, 6 + (x & 1)); }
			if (x + 2 < gridSizeX) add(index, index + 2, 8 + ((x >> 1) & 1));
			if (y + 2 < gridSizeY) add(index, index + gridSizeX * 2, 10 + ((y >> 1) & 1));
		}
	std::stable_sort(c.constraints.begin(), c.constraints.end(), [](const World::HClothConstraint& l, const World::HClothConstraint& r) { return l.color < r.color; });
	W->cloth.cloths.push_back(std::move(c)); W->cloth.dirty = true;
	return (uint32_t)W->cloth.cloths.size() - 1;
}
int mi_cloth_set_fixed_vertices(mi_world* world, uint32_t cloth, const float pos[3], const float rot[4], int moveRigid) // cloth.cpp:90-132
{
	CHECK_WORLD(MI_ERR_INVALID_ARGUMENT);
	if (cloth >= W->cloth.cloths.size() || !pos || !rot) { W->fail(MI_ERR_INVALID_ARGUMENT, "mi_cloth_set_fixed_vertices: cloth out of range"); return W->lastError; }
	W->downloadCloths();
	World::HCloth& c = W->cloth.cloths[cloth];
	Q4 q = q4(rot[0], rot[1], rot[2], rot[3]); V3 t = v3(pos[0], pos[1], pos[2]);
	auto P = [&c](u32 i) { return v3(c.pos[3 * i], c.pos[3 * i + 1], c.pos[3 * i + 2]); };
	auto xform = [&](V3 p) { return q * p + t; };
	if (moveRigid)
	{
		V3 pivot = (c.gridX % 2 == 1) ? P(c.gridX / 2) : (P(c.gridX / 2) + P(c.gridX / 2 - 1)) * 0.5f;
		V3 currentAxis = normalize(P(c.gridX - 1) - P(0));
		V3 newAxis = normalize(xform(clothParticlePosition(c, 1.f, 0.f)) - xform(clothParticlePosition(c, 0.f, 0.f)));
		V3 newPivot = xform(clothParticlePosition(c, 0.5f, 0.f));
		Q4 deltaRotation = rotateFromTo(currentAxis, newAxis);
		for (u32 y = 1; y < c.gridY; ++y)
			for (u32 x = 0; x < c.gridX; ++x)
			{
				u32 i = y * c.gridX + x;
				V3 p = deltaRotation * (P(i) - pivot) + newPivot;
				c.pos[3 * i] = p.x; c.pos[3 * i + 1] = p.y; c.pos[3 * i + 2] = p.z;
			}
	}
	for (u32 x = 0; x < c.gridX; ++x)
	{
		V3 p = xform(clothParticlePosition(c, x / (float)(c.gridX - 1), 0.f));
		c.pos[3 * x] = p.x; c.pos[3 * x + 1] = p.y; c.pos[3 * x + 2] = p.z;
	}
	W->cloth.dirty = true;
	return MI_OK;
}
int mi_cloth_set_properties(mi_world* world, uint32_t cloth, float totalMass, float stiffness, float damping, float gravityFactor)
{
	CHECK_WORLD(MI_ERR_INVALID_ARGUMENT);
	if (cloth >= W->cloth.cloths.size() || !(totalMass > 0.f)) { W->fail(MI_ERR_INVALID_ARGUMENT, "mi_cloth_set_properties: cloth out of range or mass not positive"); return W->lastError; }
	World::HCloth& c = W->cloth.cloths[cloth];
	c.totalMass = totalMass; c.stiffness = stiffness; c.damping = damping; c.gravityFactor = gravityFactor;
	W->cloth.dirty = true;
	return MI_OK;
}
int mi_set_cloth_iterations(mi_world* world, uint32_t velocityIterations, uint32_t positionIterations, uint32_t driftIterations)
{
	CHECK_WORLD(MI_ERR_INVALID_ARGUMENT);
	W->cloth.iterations[0] = velocityIterations; W->cloth.iterations[1] = positionIterations; W->cloth.iterations[2] = driftIterations;
	return MI_OK;
}
uint32_t mi_num_cloths(mi_world* world) { CHECK_WORLD(0); return (uint32_t)W->cloth.cloths.size(); }
uint32_t mi_cloth_num_particles(mi_world* world, uint32_t cloth) { CHECK_WORLD(0); return cloth < W->cloth.cloths.size() ? W->cloth.cloths[cloth].gridX * W->cloth.cloths[cloth].gridY : 0; }
int mi_cloth_read(mi_world* world, uint32_t cloth, float* positions3, float* velocities3)
{
	CHECK_WORLD(MI_ERR_INVALID_ARGUMENT);
	if (cloth >= W->cloth.cloths.size()) { W->fail(MI_ERR_INVALID_ARGUMENT, "mi_cloth_read: cloth out of range"); return W->lastError; }
	W->downloadCloths();
	const World::HCloth& c = W->cloth.cloths[cloth];
	if (positions3) memcpy(positions3, c.pos.data(), sizeof(float) * c.pos.size());
	if (velocities3) memcpy(velocities3, c.vel.data(), sizeof(float) * c.vel.size());
	return W->lastError;
}
// ---- cloth collision: the settings of the projection pass (k_cloth_collide.hip); the particle state is neither uploaded nor downloaded ----
static u32 clothFirstParticle(const World* w, u32 cloth) { u32 first = 0; for (u32 i = 0; i < cloth; ++i) first += w->cloth.cloths[i].gridX * w->cloth.cloths[i].gridY; return first; }
int mi_cloth_set_collision(mi_world* world, uint32_t cloth, const mi_cloth_collision* settings)
{
	CHECK_WORLD(MI_ERR_INVALID_ARGUMENT);
	if (cloth >= W->cloth.cloths.size()) return MI_ERR_INVALID_ARGUMENT;
	if (settings)
	{
		const mi_cloth_collision& s = *settings;
		if (!(s.thickness >= 0.f && s.thickness <= MI_FLT_MAX) || !(s.friction >= 0.f && s.friction <= MI_FLT_MAX)) return MI_ERR_INVALID_ARGUMENT;
		if ((s.flags & ~(uint32_t)(MI_CLOTH_COLLIDE_STATIC | MI_CLOTH_COLLIDE_TERRAIN)) || s.reserved[0] || s.reserved[1] || s.reserved[2]) return MI_ERR_INVALID_ARGUMENT;
	}
	W->resolvePendingFlow(); // a step that is redone is redone with the settings it ran with
	World::HCloth& c = W->cloth.cloths[cloth];
	if (c.collide && !settings)
	{
		W->cloth.numColliding--;
		if (W->cloth.contacts.p && W->cloth.contactsStride == W->cloth.stride && !W->cloth.dirty) // nothing pushes its particles off anything any more
			MI_CHECK(hipMemsetAsync(W->cloth.contacts.p + clothFirstParticle(W, cloth), 0xFF, sizeof(u32) * c.gridX * c.gridY, W->stream));
	}
	if (!c.collide && settings) W->cloth.numColliding++;
	c.collide = settings != nullptr;
	if (settings) c.collision = *settings; else c.collision = mi_cloth_collision{};
	W->cloth.collideDirty = true;
	return W->lastError;
}
int mi_cloth_get_collision(mi_world* world, uint32_t cloth, mi_cloth_collision* out, int* outEnabled)
{
	CHECK_WORLD(MI_ERR_INVALID_ARGUMENT);
	if (cloth >= W->cloth.cloths.size()) return MI_ERR_INVALID_ARGUMENT;
	const World::HCloth& c = W->cloth.cloths[cloth];
	if (out) *out = c.collision;
	if (outEnabled) *outEnabled = c.collide ? 1 : 0;
	return MI_OK;
}
int mi_cloth_read_contacts(mi_world* world, uint32_t cloth, uint32_t* outColliderPerParticle)
{
	CHECK_WORLD(MI_ERR_INVALID_ARGUMENT);
	if (cloth >= W->cloth.cloths.size() || !outColliderPerParticle) return MI_ERR_INVALID_ARGUMENT;
	const World::HCloth& c = W->cloth.cloths[cloth];
	const size_t n = (size_t)c.gridX * c.gridY;
	// none: collision off, no pass has run yet, or the particle layout has changed since the last one
	if (!c.collide || !W->cloth.contacts.p || W->cloth.contactsStride != W->cloth.stride || W->cloth.dirty) { memset(outColliderPerParticle, 0xFF, sizeof(uint32_t) * n); return W->lastError; }
	W->resolvePendingFlow();
	MI_CHECK(hipMemcpyAsync(outColliderPerParticle, W->cloth.contacts.p + clothFirstParticle(W, cloth), sizeof(uint32_t) * n, hipMemcpyDeviceToHost, W->stream));
	MI_CHECK(hipStreamSynchronize(W->stream));
	return W->lastError;
}
int mi_debug_set_cloth_collision_brute_force(mi_world* world, int on) { CHECK_WORLD(MI_ERR_INVALID_ARGUMENT); W->cloth.collideBrute = on != 0; return MI_OK; }

// ---- constraints (physics.cpp:128-333) ----
struct Trs { Q4 q; V3 p; };
static bool bodyTrs(World* w, u32 i, Trs& t)
{
	if (i >= w->bodies.size()) { w->fail(MI_ERR_INVALID_ARGUMENT, "constraint: body out of range"); return false; }
	if (w->stateOnDevice) w->downloadState();
	const World::HBody& b = w->bodies[i];
	t.q = q4(b.rot[0], b.rot[1], b.rot[2], b.rot[3]); t.p = v3(b.pos[0], b.pos[1], b.pos[2]);
	return true;
}
static V3 invPos(const Trs& t, V3 p) { return conjugate(t.q) * (p - t.p); }   // inverseTransformPosition, math.cpp:528 (scale 1)
static V3 invDir(const Trs& t, V3 d) { return conjugate(t.q) * d; }           // inverseTransformDirection, math.cpp:533
static V3 hv3(const float* p) { return v3(p[0], p[1], p[2]); }
static void put3(float* o, V3 v) { o[0] = v.x; o[1] = v.y; o[2] = v.z; }

static uint32_t pushJoint(World* w, u32 type, u32 a, u32 b, const void* pod)
{
	// both ends must be live rigid bodies of this world: the joint kernels index pose / vel with them (the reference ASSERTs the
	// components exist, physics.cpp:128-140); MI_STATIC_BODY is not a joint end
	if (a >= w->bodies.size() || b >= w->bodies.size() || w->bodies[a].removed || w->bodies[b].removed || !pod)
	{
		w->fail(MI_ERR_INVALID_ARGUMENT, "constraint: body out of range or deleted");
		return 0xFFFFFFFFu;
	}
	w->pullJointPods();
	JointSet& js = w->joints[type];
	u32 sz = MI_JOINT_POD_SIZE[type];
	js.pods.insert(js.pods.end(), (const uint8_t*)pod, (const uint8_t*)pod + sz);
	js.a.push_back(a); js.b.push_back(b); js.alive.push_back(1);
	w->jointsChanged();
	return js.count() - 1;
}

uint32_t mi_add_distance_constraint_local(mi_world* world, uint32_t a, uint32_t b, const float la[3], const float lb[3], float distance)
{
	CHECK_WORLD(0xFFFFFFFFu);
	if (!la || !lb) { W->fail(MI_ERR_INVALID_ARGUMENT, "constraint: null anchor"); return 0xFFFFFFFFu; }
	mi_distance_constraint c; memcpy(c.localAnchorA, la, 12); memcpy(c.localAnchorB, lb, 12); c.globalLength = distance;
	return pushJoint(W, MI_CONSTRAINT_DISTANCE, a, b, &c);
}
uint32_t mi_add_distance_constraint_global(mi_world* world, uint32_t a, uint32_t b, const float ga[3], const float gb[3])
{
	CHECK_WORLD(0xFFFFFFFFu);
	Trs tA, tB; if (!bodyTrs(W, a, tA) || !bodyTrs(W, b, tB)) return 0xFFFFFFFFu;
	mi_distance_constraint c; put3(c.localAnchorA, invPos(tA, hv3(ga))); put3(c.localAnchorB, invPos(tB, hv3(gb))); c.globalLength = length(hv3(ga) - hv3(gb));
	return pushJoint(W, MI_CONSTRAINT_DISTANCE, a, b, &c);
}
uint32_t mi_add_ball_constraint_local(mi_world* world, uint32_t a, uint32_t b, const float la[3], const float lb[3])
{
	CHECK_WORLD(0xFFFFFFFFu);
	if (!la || !lb) { W->fail(MI_ERR_INVALID_ARGUMENT, "constraint: null anchor"); return 0xFFFFFFFFu; }
	mi_ball_constraint c; memcpy(c.localAnchorA, la, 12); memcpy(c.localAnchorB, lb, 12);
	return pushJoint(W, MI_CONSTRAINT_BALL, a, b, &c);
}
uint32_t mi_add_ball_constraint_global(mi_world* world, uint32_t a, uint32_t b, const float g[3])
{
	CHECK_WORLD(0xFFFFFFFFu);
	Trs tA, tB; if (!bodyTrs(W, a, tA) || !bodyTrs(W, b, tB)) return 0xFFFFFFFFu;
	mi_ball_constraint c; put3(c.localAnchorA, invPos(tA, hv3(g))); put3(c.localAnchorB, invPos(tB, hv3(g)));
	return pushJoint(W, MI_CONSTRAINT_BALL, a, b, &c);
}
uint32_t mi_add_fixed_constraint_global(mi_world* world, uint32_t a, uint32_t b, const float g[3])
{
	CHECK_WORLD(0xFFFFFFFFu);
	Trs tA, tB; if (!bodyTrs(W, a, tA) || !bodyTrs(W, b, tB)) return 0xFFFFFFFFu;
	mi_fixed_constraint c; put3(c.localAnchorA, invPos(tA, hv3(g))); put3(c.localAnchorB, invPos(tB, hv3(g)));
	Q4 d = conjugate(tB.q) * tA.q;
	c.initialInvRotationDifference[0] = d.x; c.initialInvRotationDifference[1] = d.y; c.initialInvRotationDifference[2] = d.z; c.initialInvRotationDifference[3] = d.w;
	return pushJoint(W, MI_CONSTRAINT_FIXED, a, b, &c);
}
uint32_t mi_add_hinge_constraint_global(mi_world* world, uint32_t a, uint32_t b, const float anchor[3], const float axis[3], float minLimit, float maxLimit)
{
	CHECK_WORLD(0xFFFFFFFFu);
	Trs tA, tB; if (!bodyTrs(W, a, tA) || !bodyTrs(W, b, tB)) return 0xFFFFFFFFu;
	mi_hinge_constraint c; memset(&c, 0, sizeof(c));
	put3(c.localAnchorA, invPos(tA, hv3(anchor))); put3(c.localAnchorB, invPos(tB, hv3(anchor)));
	V3 axA = invDir(tA, hv3(axis));
	put3(c.localHingeAxisA, axA); put3(c.localHingeAxisB, invDir(tB, hv3(axis)));
	V3 tan = getTangent(axA), bit = cross(axA, tan);
	put3(c.localHingeTangentA, tan); put3(c.localHingeBitangentA, bit);
	put3(c.localHingeTangentB, conjugate(tB.q) * (tA.q * tan));
	c.minRotationLimit = minLimit; c.maxRotationLimit = maxLimit;
	c.motorType = MI_MOTOR_VELOCITY; c.motorVelocity = 0.f; c.maxMotorTorque = -1.f;
	return pushJoint(W, MI_CONSTRAINT_HINGE, a, b, &c);
}
uint32_t mi_add_cone_twist_constraint_global(mi_world* world, uint32_t a, uint32_t b, const float anchor[3], const float axis[3], float swingLimit, float twistLimit)
{
	CHECK_WORLD(0xFFFFFFFFu);
	Trs tA, tB; if (!bodyTrs(W, a, tA) || !bodyTrs(W, b, tB)) return 0xFFFFFFFFu;
	mi_cone_twist_constraint c; memset(&c, 0, sizeof(c));
	put3(c.localAnchorA, invPos(tA, hv3(anchor))); put3(c.localAnchorB, invPos(tB, hv3(anchor)));
	c.swingLimit = swingLimit; c.twistLimit = twistLimit;
	V3 axA = invDir(tA, hv3(axis));
	put3(c.localLimitAxisA, axA); put3(c.localLimitAxisB, invDir(tB, hv3(axis)));
	V3 tan = getTangent(axA), bit = cross(axA, tan);
	put3(c.localLimitTangentA, tan); put3(c.localLimitBitangentA, bit);
	put3(c.localLimitTangentB, conjugate(tB.q) * (tA.q * tan));
	c.swingMotorType = MI_MOTOR_VELOCITY; c.maxSwingMotorTorque = -1.f; c.twistMotorType = MI_MOTOR_VELOCITY; c.maxTwistMotorTorque = -1.f;
	return pushJoint(W, MI_CONSTRAINT_CONE_TWIST, a, b, &c);
}
uint32_t mi_add_slider_constraint_global(mi_world* world, uint32_t a, uint32_t b, const float anchor[3], const float axis[3], float minLimit, float maxLimit)
{
	CHECK_WORLD(0xFFFFFFFFu);
	Trs tA, tB; if (!bodyTrs(W, a, tA) || !bodyTrs(W, b, tB)) return 0xFFFFFFFFu;
	mi_slider_constraint c; memset(&c, 0, sizeof(c));
	put3(c.localAnchorA, invPos(tA, hv3(anchor))); put3(c.localAnchorB, invPos(tB, hv3(anchor)));
	put3(c.localAxisA, invDir(tA, hv3(axis)));
	Q4 d = conjugate(tB.q) * tA.q;
	c.initialInvRotationDifference[0] = d.x; c.initialInvRotationDifference[1] = d.y; c.initialInvRotationDifference[2] = d.z; c.initialInvRotationDifference[3] = d.w;
	c.negDistanceLimit = minLimit; c.posDistanceLimit = maxLimit;
	c.motorType = MI_MOTOR_VELOCITY; c.motorVelocity = 0.f; c.maxMotorForce = -1.f;
	return pushJoint(W, MI_CONSTRAINT_SLIDER, a, b, &c);
}

uint32_t mi_add_constraint(mi_world* world, uint32_t type, uint32_t a, uint32_t b, const void* pod)
{
	CHECK_WORLD(0xFFFFFFFFu);
	if (type >= MI_JOINT_TYPES) { W->fail(MI_ERR_INVALID_ARGUMENT, "mi_add_constraint: unknown constraint type"); return 0xFFFFFFFFu; }
	return pushJoint(W, type, a, b, pod);
}

int mi_constraint_get(mi_world* world, uint32_t type, uint32_t id, void* pod)
{
	CHECK_WORLD(MI_ERR_INVALID_ARGUMENT);
	if (type >= MI_JOINT_TYPES || id >= W->joints[type].count() || !W->joints[type].alive[id]) return MI_ERR_INVALID_ARGUMENT;
	W->pullJointPods();
	memcpy(pod, W->joints[type].pods.data() + (size_t)id * MI_JOINT_POD_SIZE[type], MI_JOINT_POD_SIZE[type]);
	return MI_OK;
}
int mi_constraint_set(mi_world* world, uint32_t type, uint32_t id, const void* pod)
{
	CHECK_WORLD(MI_ERR_INVALID_ARGUMENT);
	if (type >= MI_JOINT_TYPES || id >= W->joints[type].count() || !W->joints[type].alive[id]) return MI_ERR_INVALID_ARGUMENT;
	W->pullJointPods();
	memcpy(W->joints[type].pods.data() + (size_t)id * MI_JOINT_POD_SIZE[type], pod, MI_JOINT_POD_SIZE[type]);
	W->jointsChanged();
	return MI_OK;
}
int mi_delete_constraint(mi_world* world, uint32_t type, uint32_t id)
{
	CHECK_WORLD(MI_ERR_INVALID_ARGUMENT);
	if (type >= MI_JOINT_TYPES || id >= W->joints[type].count() || !W->joints[type].alive[id]) return MI_ERR_INVALID_ARGUMENT;
	W->pullJointPods();
	W->joints[type].alive[id] = 0; W->jointsChanged();
	return MI_OK;
}
int mi_delete_all_constraints(mi_world* world)
{
	CHECK_WORLD(MI_ERR_INVALID_ARGUMENT);
	W->pullJointPods();
	for (auto& js : W->joints) { std::fill(js.alive.begin(), js.alive.end(), 0); js.order.clear(); js.colorStart.clear(); }
	W->jointsChanged();
	return MI_OK;
}

// deleteAllConstraintsFromEntity (physics.h:264, physics.cpp:516-538): every joint that references the body
int mi_delete_all_constraints_from_body(mi_world* world, uint32_t body)
{
	CHECK_WORLD(MI_ERR_INVALID_ARGUMENT);
	if (body >= W->bodies.size()) return MI_ERR_INVALID_ARGUMENT;
	W->pullJointPods();
	for (auto& js : W->joints)
		for (u32 i = 0; i < js.count(); ++i)
			if (js.alive[i] && (js.a[i] == body || js.b[i] == body)) { js.alive[i] = 0; W->jointsChanged(); }
	return MI_OK;
}

} // extern "C"
