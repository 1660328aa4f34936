// example_ground_probe.cpp — a vehicle body over heightmap terrain reads the ground through physics_facade.hpp: its clearance with
// nearestSurface (mi_proximity, MI_PROX_TERRAIN) and how far a wheel-sized sphere drops before it touches with castSensorSphere
// (mi_sphere_cast_batch, MI_SPHERE_TERRAIN).  The terrain is the `terrain` scene's layout (2 x 2 chunks of 24 m, chunk (1, 1) a hole) with
// heights from an integer formula, so that tests/test_gpu_spherecast_terrain.py can build the same world in Python and compare.
// Prints: "clearance" distance point.xyz triangle numWithin; "blind" 0 | 1; "drop" t point.xyz normal.xyz gap; "hole" 0 | 1.
// Build: g++ -std=c++17 -Iinclude example_ground_probe.cpp -L.. -lmi_physics
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "physics_facade.hpp"

using namespace mi;

int main()
{
	try
	{
		game_scene scene;
		physics_material mat{ 0.1f, 0.8f, 1.f };
		scene.createEntity("terrain").addComponent<heightmap_collider_component>(2u, 24.f, mat);
		for (uint32_t Z = 0; Z < 2; ++Z) for (uint32_t X = 0; X < 2; ++X)
		{
			if (X == 1 && Z == 1) continue;   // the hole
			std::vector<uint16_t> heights(129 * 129);
			for (uint32_t z = 0; z < 129; ++z) for (uint32_t x = 0; x < 129; ++x)
			{
				const uint32_t gx = 128 * X + x, gz = 128 * Z + z;
				heights[129 * z + x] = (uint16_t)(12000 + 60 * gx + 35 * gz + 900 * ((7 * gx + 13 * gz) % 5));
			}
			scene.heightmapSetHeights(X, Z, heights.data());
		}
		scene.heightmapUpdate(vec3(-24.f, -2.f, -24.f), 6.f);
		auto body = scene.createEntity("chassis");
		body.addComponent<transform_component>(vec3(-5.3f, 4.f, -7.1f), quat())
			.addComponent<collider_component>(collider_component::asSphere(bounding_sphere{ vec3(0.f, 0.f, 0.f), 0.4f }, mat))
			.addComponent<rigid_body_component>(true, 1.f);

		proximity_hit near;
		if (!nearestSurface(scene, body, vec3(0.f, 0.f, 0.f), 10.f, near, true, true) || near.collider != MI_TERRAIN_COLLIDER || near.body != MI_STATIC_BODY) std::abort();
		std::printf("clearance %.7f %.7f %.7f %.7f %u %u\n", near.distance, near.point.x, near.point.y, near.point.z, near.triangle, near.numWithin);
		std::printf("blind %d\n", nearestSurface(scene, body, vec3(0.f, 0.f, 0.f), 10.f, near) ? 1 : 0);          // without the terrain nothing is near
		if (countWithin(scene, vec3(-5.3f, 4.f, -7.1f), 10.f, true) != 2u) std::abort();                           // the chassis and the ground
		sphere_hit hit;
		const vec3 wheel(0.6f, -0.2f, 0.f), down(0.f, -1.f, 0.f);
		if (!castSensorSphere(scene, body, wheel, down, 0.35f, 20.f, hit, true, true) || hit.unresolved || hit.collider != MI_TERRAIN_COLLIDER) std::abort();
		std::printf("drop %.7f %.7f %.7f %.7f %.7f %.7f %.7f %.7g\n", hit.distance, hit.point.x, hit.point.y, hit.point.z, hit.normal.x, hit.normal.y, hit.normal.z, hit.gap);
		if (castSensorSphere(scene, body, wheel, down, 0.35f, 20.f, hit)) std::abort();                              // and nothing under the wheel
		std::printf("hole %d\n", castSphere(scene, vec3(12.f, 8.f, 12.f), down, 0.35f, 50.f, hit, true) ? 1 : 0);   // through the hole: free
		return 0;
	}
	catch (const std::exception& e) { std::fprintf(stderr, "error: %s\n", e.what()); return 1; }
}
