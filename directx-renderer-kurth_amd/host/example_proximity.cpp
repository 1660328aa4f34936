// example_proximity.cpp — a proximity sensor on a ragdoll's pelvis through physics_facade.hpp's nearestSurface / countWithin
// (mi_proximity): the pelvis sphere between a box and an octahedron hull.  Prints per sensor: name, distance, world normal; per count:
// name, number of colliders (tests/test_gpu_proximity.py checks them).
// Build: g++ -std=c++17 -Iinclude example_proximity.cpp -L.. -lmi_physics
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "physics_facade.hpp"

using namespace mi;

static void print(const char* name, const proximity_hit& h) { std::printf("%s %.6f %.6f %.6f %.6f\n", name, h.distance, h.normal.x, h.normal.y, h.normal.z); }

int main()
{
	try
	{
		game_scene scene;
		physics_material mat{ 0.1f, 0.5f, 1.f };
		scene.createEntity("box")   // its nearest face at x = 1
			.addComponent<transform_component>(vec3(2.f, 1.f, 0.f), quat())
			.addComponent<collider_component>(collider_component::asAABB(bounding_box::fromCenterRadius(vec3(0.f, 0.f, 0.f), vec3(1.f, 1.f, 1.f)), mat));
		const float a = 0.4f;       // an octahedron with its tip at (0, 1, -0.8)
		const std::vector<vec3> verts = { vec3(a, 0, 0), vec3(-a, 0, 0), vec3(0, a, 0), vec3(0, -a, 0), vec3(0, 0, a), vec3(0, 0, -a) };
		std::vector<uint32_t> tris;
		for (uint32_t k = 0; k < 8; ++k)
		{
			const uint32_t x = (k & 1) ? 1u : 0u, y = (k & 2) ? 3u : 2u, z = (k & 4) ? 5u : 4u;
			const bool even = (((k & 1) != 0) + ((k & 2) != 0) + ((k & 4) != 0)) % 2 == 0;   // an even number of negative axes: (x, y, z) is outward
			tris.insert(tris.end(), { x, even ? y : z, even ? z : y });
		}
		const uint32_t geometry = scene.allocateBoundingHullGeometry(verts, tris);
		scene.createEntity("hull")
			.addComponent<transform_component>(vec3(0.f, 1.f, -1.2f), quat())
			.addComponent<collider_component>(collider_component::asHull(bounding_hull{ quat(), vec3(0.f, 0.f, 0.f), geometry }, mat));
		auto pelvis = scene.createEntity("pelvis");
		pelvis.addComponent<transform_component>(vec3(0.f, 1.f, 0.f), quat())
			.addComponent<collider_component>(collider_component::asSphere(bounding_sphere{ vec3(0.f, 0.f, 0.f), 0.15f }, mat))
			.addComponent<rigid_body_component>(true, 1.f);

		proximity_hit hit;
		// at the pelvis's centre: without exclusion the sensor reports its own carrier, from inside
		if (!nearestSurface(scene, pelvis, vec3(0.f, 0.f, 0.f), 5.f, hit, false) || hit.body != pelvis.body()) std::abort();
		print("self", hit);
		if (!nearestSurface(scene, pelvis, vec3(0.f, 0.f, 0.f), 5.f, hit) || hit.body != MI_STATIC_BODY || hit.numWithin != 2u) std::abort();
		print("hull", hit);
		if (!nearestSurface(scene, pelvis, vec3(0.6f, 0.f, 0.f), 5.f, hit)) std::abort();   // a sensor on the pelvis's right side
		print("box", hit);
		if (nearestSurface(scene, pelvis, vec3(0.f, 0.f, 0.f), 0.5f, hit)) std::abort();    // nothing within half a metre
		std::printf("count %u\n", countWithin(scene, vec3(0.f, 1.f, 0.f), 0.9f));           // the pelvis and the hull
		std::printf("count_near %u\n", countWithin(scene, vec3(0.f, 3.f, 0.f), 0.5f));      // free space: a spawn point
		std::printf("count_all %u\n", countWithin(scene, vec3(0.f, 1.f, 0.f), 1.05f));
		return 0;
	}
	catch (const std::exception& e) { std::fprintf(stderr, "error: %s\n", e.what()); return 1; }
}
