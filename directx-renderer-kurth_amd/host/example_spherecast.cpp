// example_spherecast.cpp — a ragdoll's foot probe through physics_facade.hpp's castSensorSphere / castSphere (mi_sphere_cast_batch):
// the foot hangs over a 10 cm gap between two floor slabs, the ground 55 cm below them.  A ray sensor looks down through the gap and
// reports the ground; a sphere of the foot's size does not fit and stops on the edge of a slab.  Prints per probe: name, t, world
// normal (tests/test_gpu_spherecast.py checks them).
// Build: g++ -std=c++17 -Iinclude example_spherecast.cpp -L.. -lmi_physics
#include <cstdio>
#include <cstdlib>
#include "physics_facade.hpp"

using namespace mi;

static void print(const char* name, float t, vec3 n) { std::printf("%s %.6f %.6f %.6f %.6f\n", name, t, n.x, n.y, n.z); }

int main()
{
	try
	{
		game_scene scene;
		physics_material mat{ 0.1f, 0.5f, 1.f };
		scene.createEntity("left slab")     // top at y = 0.55, x in [-1.05, -0.05]
			.addComponent<transform_component>(vec3(-0.55f, 0.5f, 0.f), quat())
			.addComponent<collider_component>(collider_component::asAABB(bounding_box::fromCenterRadius(vec3(0.f, 0.f, 0.f), vec3(0.5f, 0.05f, 0.5f)), mat));
		scene.createEntity("right slab")    // x in [0.05, 1.05]
			.addComponent<transform_component>(vec3(0.55f, 0.5f, 0.f), quat())
			.addComponent<collider_component>(collider_component::asAABB(bounding_box::fromCenterRadius(vec3(0.f, 0.f, 0.f), vec3(0.5f, 0.05f, 0.5f)), mat));
		scene.createEntity("ground")        // top at y = 0
			.addComponent<transform_component>(vec3(0.f, -0.5f, 0.f), quat())
			.addComponent<collider_component>(collider_component::asAABB(bounding_box::fromCenterRadius(vec3(0.f, 0.f, 0.f), vec3(5.f, 0.5f, 5.f)), mat));
		auto foot = scene.createEntity("foot");
		foot.addComponent<transform_component>(vec3(0.f, 1.f, 0.f), quat())
			.addComponent<collider_component>(collider_component::asSphere(bounding_sphere{ vec3(0.f, 0.f, 0.f), 0.05f }, mat))
			.addComponent<rigid_body_component>(true, 1.f);

		const vec3 probe(0.01f, 0.f, 0.f), down(0.f, -1.f, 0.f);   // a centimetre off the gap's middle, so that one slab is the nearer
		sensor_hit seen;
		if (!castSensorRay(scene, foot, ray{ probe, down }, 5.f, seen)) std::abort();
		print("ray", seen.distance, seen.normal);                  // through the gap, onto the ground
		sphere_hit hit;
		if (!castSensorSphere(scene, foot, probe, down, 0.03f, 5.f, hit) || hit.unresolved) std::abort();
		print("thin", hit.distance, hit.normal);                   // a 3 cm sphere still fits through
		if (!castSensorSphere(scene, foot, probe, down, 0.08f, 5.f, hit) || hit.unresolved || hit.body != MI_STATIC_BODY) std::abort();
		print("foot", hit.distance, hit.normal);                   // the foot does not: it comes to rest on the right slab's edge
		if (!castSensorSphere(scene, foot, probe, down, 0.08f, 5.f, hit, false) || hit.body != foot.body() || !(hit.gap < 0.f)) std::abort();
		print("self", hit.distance, hit.normal);                   // without exclusion the probe starts inside its carrier: t = 0
		if (!castSphere(scene, vec3(0.5f, 1.f, 0.f), down, 0.08f, 5.f, hit)) std::abort();
		print("slab", hit.distance, hit.normal);                   // a world-space cast beside the foot: flat on the right slab
		if (castSphere(scene, vec3(0.5f, 1.f, 0.f), down, 0.08f, 0.3f, hit)) std::abort();   // nothing within 30 cm
		return 0;
	}
	catch (const std::exception& e) { std::fprintf(stderr, "error: %s\n", e.what()); return 1; }
}
