// example_cloth_drape.cpp — cloth collision through physics_facade.hpp's setClothCollision / clothContacts (mi_cloth_set_collision): a
// sheet held by its upper row is dropped over a static sphere that stands on a ground box.  Prints the lowest particle and the number
// of particles that were pushed off a collider in the last step (tests/test_gpu_cloth_collision.py checks them).
// Build: g++ -std=c++17 -Iinclude example_cloth_drape.cpp -L.. -lmi_physics
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
		scene.createEntity("ground")   // its top face at y = 0
			.addComponent<transform_component>(vec3(0.f, -1.f, 0.f), quat())
			.addComponent<collider_component>(collider_component::asAABB(bounding_box::fromCenterRadius(vec3(0.f, 0.f, 0.f), vec3(10.f, 1.f, 10.f)), mat));
		scene.createEntity("sphere")
			.addComponent<transform_component>(vec3(0.f, 1.f, 0.f), quat())
			.addComponent<collider_component>(collider_component::asSphere(bounding_sphere{ vec3(0.f, 0.f, 0.f), 1.f }, mat));
		scene.createEntity("ball")     // (a world steps once it has a rigid body)
			.addComponent<transform_component>(vec3(6.f, 0.5f, 6.f), quat())
			.addComponent<collider_component>(collider_component::asSphere(bounding_sphere{ vec3(0.f, 0.f, 0.f), 0.5f }, mat))
			.addComponent<rigid_body_component>(false, 1.f);
		auto sheet = scene.createEntity("sheet");
		sheet.addComponent<transform_component>(vec3(0.f, 2.3f, 1.5f), quat()).addComponent<cloth_component>(3.f, 3.f, 24u, 24u, 2.f);
		const float thickness = 0.05f;
		sheet.setClothCollision(thickness, 0.5f, MI_CLOTH_COLLIDE_STATIC);

		physics_settings settings; memory_arena arena; float timer = 0.f;
		for (int frame = 0; frame < 240; ++frame) physicsStep(scene, arena, timer, settings, 1.f / 60.f);

		float lowest = 1e30f;
		for (const vec3& p : sheet.clothPositions()) if (p.y < lowest) lowest = p.y;
		uint32_t touching = 0;
		for (uint32_t c : sheet.clothContacts()) if (c != 0xFFFFFFFFu) ++touching;
		std::printf("lowest particle y = %.6f\ntouching particles = %u\n", lowest, touching);
		return 0;
	}
	catch (const std::exception& e) { std::fprintf(stderr, "error: %s\n", e.what()); return 1; }
}
