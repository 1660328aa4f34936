// example_overlap.cpp — overlap queries through physics_facade.hpp's overlapSphere / overlapBox / overlapVolume (mi_overlap_batch): a
// row of five crates on a floor and a gripper body over the third.  Prints per query: name, total count, then collider:body pairs
// (body -1 for a static collider); tests/test_gpu_overlap.py asks Python for the same scene and compares the lists.
// Build: g++ -std=c++17 -Iinclude example_overlap.cpp -L.. -lmi_physics
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "physics_facade.hpp"

using namespace mi;

static void print(const char* name, uint32_t total, const std::vector<overlap_hit>& hits)
{
	std::printf("%s %u", name, total);
	for (const overlap_hit& h : hits) std::printf(" %u:%d", h.collider, h.body == MI_STATIC_BODY ? -1 : (int)h.body);
	std::printf("\n");
}

int main()
{
	try
	{
		game_scene scene;
		physics_material mat{ 0.1f, 0.5f, 1.f };
		scene.createEntity("floor")
			.addComponent<transform_component>(vec3(0.f, -0.5f, 0.f), quat())
			.addComponent<collider_component>(collider_component::asAABB(bounding_box::fromCenterRadius(vec3(0.f, 0.f, 0.f), vec3(10.f, 0.5f, 10.f)), mat));
		for (int k = 0; k < 5; ++k)   // crates of 1 m at x = -4, -2, 0, 2, 4, resting on the floor: bodies 0 .. 4
			scene.createEntity("crate")
				.addComponent<transform_component>(vec3(-4.f + 2.f * k, 0.5f, 0.f), quat())
				.addComponent<collider_component>(collider_component::asOBB(bounding_oriented_box{ quat(), vec3(0.f, 0.f, 0.f), vec3(0.5f, 0.5f, 0.5f) }, mat))
				.addComponent<rigid_body_component>(true, 1.f);
		auto gripper = scene.createEntity("gripper");   // body 5: a palm over the middle crate, turned a quarter about y
		gripper.addComponent<transform_component>(vec3(0.f, 1.3f, 0.f), quat(0.f, 0.70710678f, 0.f, 0.70710678f))
			.addComponent<collider_component>(collider_component::asAABB(bounding_box::fromCenterRadius(vec3(0.f, 0.f, 0.f), vec3(0.4f, 0.1f, 0.4f)), mat))
			.addComponent<rigid_body_component>(true, 1.f);

		std::vector<overlap_hit> hits;
		print("blast", overlapSphere(scene, vec3(1.f, 0.5f, 0.f), 1.2f, hits), hits);                             // a blast radius between crates 2 and 3: both, the palm above and the floor
		print("pad", overlapBox(scene, vec3(-3.f, 0.25f, 0.f), quat(), vec3(1.6f, 0.25f, 0.6f), hits), hits);     // which bodies stand on this pad
		print("spawn", overlapSphere(scene, vec3(0.f, 4.f, 0.f), 0.5f, hits), hits);                              // a free spawn point
		// the gripper's span: a box under the palm, in the palm's frame; the palm itself is not reported
		const collider_component span = collider_component::asAABB(bounding_box::fromCenterRadius(vec3(0.f, 0.f, 0.f), vec3(0.3f, 0.3f, 0.3f)), mat);
		print("span", overlapVolume(scene, gripper, span, vec3(0.f, -0.35f, 0.f), quat(), hits), hits);
		print("span_self", overlapVolume(scene, gripper, span, vec3(0.f, -0.35f, 0.f), quat(), hits, false), hits);
		const collider_component rod = collider_component::asCapsule(bounding_capsule{ vec3(-5.f, 0.f, 0.f), vec3(5.f, 0.f, 0.f), 0.1f }, mat);
		print("rod", overlapVolume(scene, rod, vec3(0.f, 0.5f, 0.f), quat(), hits, 3u), hits);                    // through all five crates, the first three listed
		return 0;
	}
	catch (const std::exception& e) { std::fprintf(stderr, "error: %s\n", e.what()); return 1; }
}
