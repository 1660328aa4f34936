// example_depenetrate.cpp — contact queries through physics_facade.hpp's contactsOfVolume / penetrationOf / depenetrate
// (mi_contact_query_batch) and castSphere (mi_sphere_cast_batch): the two halves of a kinematic character controller.  A character
// capsule is dropped into a corner made of a static floor box, a wall turned by 45 degrees (an OBB) and a convex hull; it is pushed
// free along the deepest contact's normal, then swept on with a sphere cast.  Prints
//   start <contacts> <deepest |depth|>      where it was dropped
//   slop <s> / iterations <n>                the push-out's budget
//   free <contacts> <deepest |depth|> <iterations used>
//   position <x> <y> <z>                     where it came free
//   sweep <hit> <distance>                   how far it can slide on along the wall
// tests/test_gpu_contact_query.py builds the same corner in Python and asks about the two positions.
// Build: g++ -std=c++17 -Iinclude example_depenetrate.cpp -L.. -lmi_physics
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
		physics_material mat{ 0.1f, 0.5f, 1.f };
		scene.createEntity("floor")
			.addComponent<transform_component>(vec3(0.f, -0.5f, 0.f), quat())
			.addComponent<collider_component>(collider_component::asAABB(bounding_box::fromCenterRadius(vec3(0.f, 0.f, 0.f), vec3(4.f, 0.5f, 4.f)), mat));
		scene.createEntity("wall")   // an axis-aligned box on an entity turned by 45 degrees about y: an OBB in the world
			.addComponent<transform_component>(vec3(2.f, 1.f, 0.f), quat(0.f, 0.38268343f, 0.f, 0.92387953f))
			.addComponent<collider_component>(collider_component::asAABB(bounding_box::fromCenterRadius(vec3(0.f, 0.f, 0.f), vec3(0.5f, 1.f, 2.f)), mat));
		const float hx = 1.f, hy = 0.5f, hz = 0.5f;
		const std::vector<vec3> vertices = { vec3(-hx, -hy, -hz), vec3(hx, -hy, -hz), vec3(hx, hy, -hz), vec3(-hx, hy, -hz), vec3(-hx, -hy, hz), vec3(hx, -hy, hz), vec3(hx, hy, hz), vec3(-hx, hy, hz) };
		const std::vector<uint32_t> triangles = { 0, 2, 1, 0, 3, 2, 4, 5, 6, 4, 6, 7, 0, 1, 5, 0, 5, 4, 2, 3, 7, 2, 7, 6, 1, 2, 6, 1, 6, 5, 0, 4, 7, 0, 7, 3 };
		const uint32_t geometry = scene.allocateBoundingHullGeometry(vertices, triangles);
		scene.createEntity("block")
			.addComponent<transform_component>(vec3(0.3f, 0.5f, -1.2f), quat())
			.addComponent<collider_component>(collider_component::asHull(bounding_hull{ quat(), vec3(0.f, 0.f, 0.f), geometry }, mat));

		const collider_component character = collider_component::asCapsule(bounding_capsule{ vec3(0.f, -0.5f, 0.f), vec3(0.f, 0.5f, 0.f), 0.4f }, mat);
		vec3 position(1.f, 0.7f, -0.4f);   // feet 0.2 in the floor, a shoulder in the wall, the back in the block
		const float slop = 0.01f;          // EPA stops refining a polytope at 0.01: no depth of a GJK pair is known better than that
		const uint32_t iterations = 16u;

		std::vector<volume_contact> contacts;
		volume_penetration p = penetrationOf(scene, character, position, quat());
		std::printf("start %u %.9g\n", contactsOfVolume(scene, character, position, quat(), contacts), p.depth);
		std::printf("slop %.9g\niterations %u\n", slop, iterations);
		float remaining = 0.f;
		const uint32_t used = depenetrate(scene, character, position, quat(), iterations, slop, &remaining);
		std::printf("free %u %.9g %u\n", contactsOfVolume(scene, character, position, quat(), contacts), remaining, used);
		std::printf("position %.9g %.9g %.9g\n", position.x, position.y, position.z);
		// on from there: how far can the character slide along the wall before it meets the block?  Its lower sphere, a little slimmer
		// and lifted (it rests against wall and floor: at full size every cast along them starts in touch)
		sphere_hit hit;
		const bool blocked = castSphere(scene, vec3(position.x, position.y - 0.5f + 0.05f, position.z), vec3(-0.70710678f, 0.f, -0.70710678f), 0.35f, 10.f, hit);
		std::printf("sweep %d %.9g\n", blocked ? 1 : 0, blocked ? hit.distance : 10.f);
		return remaining <= slop ? 0 : 2;
	}
	catch (const std::exception& e) { std::fprintf(stderr, "error: %s\n", e.what()); return 1; }
}
