// example_sensor.cpp — range sensors fixed to a rigid body through physics_facade.hpp's castSensorRay (mi_raycast_sensors): a kinematic
// "robot" sphere turned by 90 degrees about y over a platform, a pillar in front of it and a sloped heightmap beside the platform.
// Prints one line per sensor: name, distance, hit point, world normal (tests/test_gpu_raycast_sensors.py checks them).
// Build: g++ -std=c++17 -Iinclude example_sensor.cpp -L.. -lmi_physics
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "physics_facade.hpp"

using namespace mi;

static void print(const char* name, const sensor_hit& h)
{
	std::printf("%s %.6f %.6f %.6f %.6f %.6f %.6f %.6f\n", name, h.distance, h.point.x, h.point.y, h.point.z, h.normal.x, h.normal.y, h.normal.z);
}

int main()
{
	try
	{
		game_scene scene;
		physics_material mat{ 0.1f, 0.5f, 1.f };
		scene.createEntity("platform")
			.addComponent<transform_component>(vec3(0.f, -1.f, 0.f), quat())
			.addComponent<collider_component>(collider_component::asAABB(bounding_box::fromCenterRadius(vec3(0.f, 0.f, 0.f), vec3(5.f, 1.f, 5.f)), mat));
		scene.createEntity("pillar")
			.addComponent<transform_component>(vec3(0.f, 2.f, -3.f), quat())
			.addComponent<collider_component>(collider_component::asAABB(bounding_box::fromCenterRadius(vec3(0.f, 0.f, 0.f), vec3(1.f, 3.f, 0.5f)), mat));
		const float s = std::sqrt(0.5f);
		auto robot = scene.createEntity("robot");   // turned by 90 degrees about y: its +x looks along the world's -z
		robot.addComponent<transform_component>(vec3(0.f, 2.f, 0.f), quat(0.f, s, 0.f, s))
			.addComponent<collider_component>(collider_component::asSphere(bounding_sphere{ vec3(0.f, 0.f, 0.f), 0.5f }, mat))
			.addComponent<rigid_body_component>(true, 1.f);
		auto scout = scene.createEntity("scout");   // beside the platform, over the terrain
		scout.addComponent<transform_component>(vec3(20.f, 2.f, 0.f), quat())
			.addComponent<collider_component>(collider_component::asSphere(bounding_sphere{ vec3(0.f, 0.f, 0.f), 0.5f }, mat))
			.addComponent<rigid_body_component>(true, 1.f);
		{	// one chunk of 64 m whose heights rise along x
			scene.createEntity("terrain").addComponent<heightmap_collider_component>(1u, 64.f, mat);
			std::vector<uint16_t> heights(129 * 129);
			for (int z = 0; z < 129; ++z) for (int x = 0; x < 129; ++x) heights[129 * z + x] = (uint16_t)(400 * x);
			scene.heightmapSetHeights(0, 0, heights.data());
			scene.heightmapUpdate(vec3(-32.f, -12.f, -32.f), 8.f);
		}

		sensor_hit hit;
		// from the centre of the robot along its +x: without exclusion the sensor sees its own carrier, at distance 0
		if (!castSensorRay(scene, robot, ray{ vec3(0.f, 0.f, 0.f), vec3(1.f, 0.f, 0.f) }, 100.f, hit, false) || hit.body != robot.body()) std::abort();
		print("self", hit);
		if (!castSensorRay(scene, robot, ray{ vec3(0.f, 0.f, 0.f), vec3(1.f, 0.f, 0.f) }, 100.f, hit) || hit.body != MI_STATIC_BODY) std::abort();
		print("pillar", hit);
		if (castSensorRay(scene, robot, ray{ vec3(0.f, 0.f, 0.f), vec3(1.f, 0.f, 0.f) }, 2.f, hit)) std::abort(); // out of range
		if (!castSensorRay(scene, robot, ray{ vec3(0.f, 0.f, 0.f), vec3(0.f, -1.f, 0.f) }, 100.f, hit)) std::abort();
		print("ground", hit);
		if (castSensorRay(scene, scout, ray{ vec3(0.f, 0.f, 0.f), vec3(0.f, -1.f, 0.f) }, 100.f, hit)) std::abort(); // nothing but terrain below, and the terrain was not asked for
		if (!castSensorRay(scene, scout, ray{ vec3(0.f, 0.f, 0.f), vec3(0.f, -1.f, 0.f) }, 100.f, hit, true, true) || hit.collider != MI_TERRAIN_COLLIDER) std::abort();
		print("terrain", hit);
		return 0;
	}
	catch (const std::exception& e) { std::fprintf(stderr, "error: %s\n", e.what()); return 1; }
}
