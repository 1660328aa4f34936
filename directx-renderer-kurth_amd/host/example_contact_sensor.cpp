// example_contact_sensor.cpp — the load on a resting body through physics_facade.hpp's contactImpulse (mi_contact_sensors): a sphere at
// rest on a static box under gravity, a second sphere resting on top of it.  Prints one line per reading: name, normal impulse per step,
// the linear impulse, contacts, manifolds, strongest partner (tests/test_gpu_contact_sensors.py checks them against m g dt).
// Build: g++ -std=c++17 -Iinclude example_contact_sensor.cpp -L.. -lmi_physics
#include <cstdio>
#include "physics_facade.hpp"

using namespace mi;

static void print(const char* name, const contact_impulse& c)
{
	std::printf("%s %.9g %.9g %.9g %.9g %u %u %u\n", name, c.normalImpulse, c.impulse.x, c.impulse.y, c.impulse.z, c.numContacts, c.numManifolds, c.strongestPartner);
}

#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "unexpected reading: %s\n", #cond); return 2; } } while (0)

int main()
{
	try
	{
		game_scene scene;
		physics_material mat{ 0.f, 0.5f, 1000.f };
		scene.createEntity("floor")
			.addComponent<transform_component>(vec3(0.f, -0.5f, 0.f), quat())
			.addComponent<collider_component>(collider_component::asAABB(bounding_box::fromCenterRadius(vec3(0.f, 0.f, 0.f), vec3(4.f, 0.5f, 4.f)), mat));
		auto lower = scene.createEntity("lower");
		lower.addComponent<transform_component>(vec3(0.f, 0.25f, 0.f), quat())
			.addComponent<collider_component>(collider_component::asSphere(bounding_sphere{ vec3(0.f, 0.f, 0.f), 0.25f }, mat))
			.addComponent<rigid_body_component>(false, 1.f, 0.f, 0.f);
		auto upper = scene.createEntity("upper");
		upper.addComponent<transform_component>(vec3(0.f, 0.75f, 0.f), quat())
			.addComponent<collider_component>(collider_component::asSphere(bounding_sphere{ vec3(0.f, 0.f, 0.f), 0.25f }, mat))
			.addComponent<rigid_body_component>(false, 1.f, 0.f, 0.f);

		EXPECT(!contactImpulse(lower).valid); // no step yet: no reading
		physics_settings settings; settings.fixedFrameRate = false;
		memory_arena arena; float timer = 0.f;
		for (int i = 0; i < 240; ++i) physicsStep(scene, arena, timer, settings, 1.f / 120.f);

		contact_impulse c = contactImpulse(lower);
		EXPECT(c.valid && c.numManifolds == 2);
		print("lower", c);
		c = contactImpulse(lower, MI_CONTACT_STATIC);
		EXPECT(c.valid && c.strongestPartner == MI_STATIC_BODY);
		print("lower_floor", c);   // the floor carries both spheres
		c = contactImpulse(lower, MI_CONTACT_DYNAMIC);
		EXPECT(c.valid && c.strongestPartner == upper.body());
		print("lower_upper", c);
		c = contactImpulse(upper, MI_CONTACT_DYNAMIC | MI_CONTACT_STATIC, lower.body(), 1u);
		EXPECT(c.valid && c.numManifolds == 0); // its one partner is excluded
		c = contactImpulse(upper);
		EXPECT(c.valid && c.strongestPartner == lower.body());
		print("upper", c);
		return 0;
	}
	catch (const std::exception& e) { std::fprintf(stderr, "error: %s\n", e.what()); return 1; }
}
